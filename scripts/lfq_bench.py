#!/usr/bin/env python3
"""Label-free quantification (sage_hip_lfq) at a realistic size: N files x S MS1 spectra x P peaks, Q quantified peptides
(windows: 3 charges x 3 isotopes x forward/decoy per peptide).  Prints one JSON line: the HIP-event times of the stages
(feature map, MS1 sort, traces, integration), the call's wall time, and the restatement's CPU time per peak on a slice.

    python scripts/lfq_bench.py [--files 10 --ms1 6000 --peaks 4000 --peptides 40000 --steps 3] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sage_amd import _lib as L  # noqa: E402
from sage_amd.api import ALIGNMENT_DTYPE, LfqSettings, RawBatch, lfq  # noqa: E402

PROTON, NEUTRON = 1.0072764, 1.00335


def workload(files, ms1, peaks, peptides, seed=0, sigma=0.0008):
    """Peptides eluting as Gaussians (sigma: fraction of the run), their 3 charges x 3 isotopes as MS1 peaks, the rest of each
    spectrum uniform noise.  Every file: RT = run fraction (alignment slope 1)."""
    rng = np.random.default_rng(seed)
    mass = rng.uniform(800.0, 3500.0, peptides).astype(np.float32)
    apex = rng.uniform(0.03, 0.97, peptides).astype(np.float32)
    order = np.argsort(apex)
    mass, apex = mass[order], apex[order]
    f = np.zeros(peptides, dtype=L.FEATURE_DTYPE)
    f["peptide_idx"] = np.arange(peptides)
    f["label"] = 1
    f["calcmass"] = mass
    f["file_id"] = rng.integers(0, files, peptides)
    art, pq = apex.copy(), np.zeros(peptides, np.float32)
    carbon = (mass / 14.5).astype(np.uint16)
    sulfur = rng.integers(0, 3, peptides).astype(np.uint16)
    al = np.zeros(files, ALIGNMENT_DTYPE)
    for i in range(files):
        al[i] = (i, 1.0, 1.0, 0.0)
    z = np.array([2, 3, 4])
    iso = np.arange(3)
    batches = []
    for fi in range(files):
        t = ((np.arange(ms1) + 0.5) / ms1).astype(np.float32)
        lo = np.searchsorted(apex, t - 3 * sigma)
        hi = np.searchsorted(apex, t + 3 * sigma)
        off = np.zeros(ms1 + 1, np.uint64)
        off[1:] = np.cumsum(np.full(ms1, peaks, np.uint64))
        mz = np.empty(ms1 * peaks, np.float32)
        it = np.empty(ms1 * peaks, np.float32)
        for s in range(ms1):
            p = np.arange(lo[s], hi[s])
            sig = ((mass[p, None, None] + iso[None, None, :] * NEUTRON) / z[None, :, None] + PROTON).reshape(-1)[:peaks]
            h = (1e6 * np.exp(-0.5 * ((t[s] - apex[p]) / sigma) ** 2))[:, None, None] * np.array([1.0, 0.8, 0.4])[None, None, :]
            h = np.broadcast_to(h, (len(p), 3, 3)).reshape(-1)[:peaks]
            n = peaks - len(sig)
            m = np.concatenate([sig, rng.uniform(300.0, 1600.0, n)]).astype(np.float32)
            v = np.concatenate([h, rng.lognormal(7.0, 1.0, n)]).astype(np.float32)
            k = np.argsort(m, kind="stable")
            a = s * peaks
            mz[a:a + peaks], it[a:a + peaks] = m[k], v[k]
        b = RawBatch.from_arrays([""] * ms1, off, mz, it, np.zeros(ms1, np.float32), np.zeros(ms1, np.uint8),
                                 np.full(ms1, np.nan, np.float32), np.full(ms1, np.nan, np.float32), t,
                                 np.full(ms1, np.nan, np.float32), np.full(ms1, fi, np.uint32))
        batches.append(b)
    return f, art, pq, al, batches, carbon, sulfur


def cpu_slice(f, art, pq, al, batches, carbon, sulfur, n_pep=2000, n_spec=4):
    """the restatement's time per MS1 peak on a slice (its feature map holds n_pep peptides)"""
    import lfq_reference as R
    sel = slice(0, n_pep)
    feats = dict(peptide_idx=f["peptide_idx"][sel], label=f["label"][sel], calcmass=f["calcmass"][sel], file_id=f["file_id"][sel],
                 aligned_rt=art[sel], peptide_q=pq[sel])
    fmap = R.build_feature_map(R.default_settings(), (2, 4), feats)
    b = batches[0]
    mid = float(np.median(art[sel]))
    s0 = int(np.searchsorted(b.scan_start_time, mid))
    spectra = []
    for i in range(s0, s0 + n_spec):
        lo, hi = int(b.peak_off[i]), int(b.peak_off[i + 1])
        m, it = R.process_ms1(b.mz[lo:hi], b.intensities[lo:hi])
        spectra.append((0, np.float32(b.scan_start_time[i]), m, it))
    iso = lambda p: R.peptide_isotopes(int(carbon[p]), int(sulfur[p]))
    t0 = time.time()
    grids = R.trace(fmap, spectra, [tuple(a) for a in al.tolist()], len(al), True, iso)
    t_trace = time.time() - t0
    t0 = time.time()
    R.quantify(R.default_settings(), (2, 4), None, None, None, len(al), None, grids=grids)
    t_int = time.time() - t0
    n_peaks = sum(len(s[2]) for s in spectra)
    return {"cpu_slice_peptides": n_pep, "cpu_slice_peaks": n_peaks, "cpu_trace_us_per_peak": t_trace / n_peaks * 1e6,
            "cpu_slice_grids": len(grids), "cpu_integrate_ms_per_grid": t_int / max(len(grids), 1) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=10)
    ap.add_argument("--ms1", type=int, default=6000)
    ap.add_argument("--peaks", type=int, default=4000)
    ap.add_argument("--peptides", type=int, default=40000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    t0 = time.time()
    f, art, pq, al, batches, carbon, sulfur = workload(a.files, a.ms1, a.peaks, a.peptides)
    gen_s = time.time() - t0
    st = LfqSettings()
    res = lfq(f, None, art, pq, al, batches, carbon, sulfur, st, (2, 4))  # warm-up
    runs = []
    for _ in range(a.steps):
        t0 = time.time()
        res = lfq(f, None, art, pq, al, batches, carbon, sulfur, st, (2, 4))
        runs.append(dict(res.stage_ms, wall_ms=(time.time() - t0) * 1e3))
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    out = {"workload": {"files": a.files, "ms1_per_file": a.ms1, "peaks_per_spectrum": a.peaks, "peptides": a.peptides,
                        "ms1_peaks": a.files * a.ms1 * a.peaks, "windows": res.n_windows}, "generate_s": gen_s,
           "contributions": res.n_contributions, "grids": len(res.peptide_idx), "peaks_found": int(res.has_peak.sum()),
           "passing": res.passing, "median_ms": med, "runs": runs}
    if not a.no_cpu:
        out.update(cpu_slice(f, art, pq, al, batches, carbon, sulfur))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
