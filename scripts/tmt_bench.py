#!/usr/bin/env python3
"""TMT reporter-ion quantification (sage_hip_tmt) at a user's size: an SPS-MS3 run of N files x S MS3 spectra x P peaks
(level 3: raw peaks, no sort) and a level-2 run of N files x S MS2 spectra x P2 raw peaks (device preprocessing first).
Prints one JSON line: per level the median HIP-event stage times (upload or process, extraction, whole call) and wall time,
and the restatement's CPU time per spectrum on a slice.

    python scripts/tmt_bench.py [--files 12 --spectra 40000 --peaks 500 --ms2-peaks 400 --steps 3] [--no-cpu]
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

from sage_amd.api import Isobaric, RawBatch, tmt  # noqa: E402


def workload(files, spectra, peaks, labels, seed=0, sort=False):
    """Per spectrum: the reporter cluster (90 % of labels present, +-4 ppm) and uniform peaks over 100-2000 m/z.  Level 3
    spectra are left in m/z order as written by instruments; the kernel does not rely on it."""
    rng = np.random.default_rng(seed)
    out = []
    nl = len(labels)
    for f in range(files):
        n = spectra * peaks
        mz = rng.uniform(100.0, 2000.0, n).astype(np.float32).reshape(spectra, peaks)
        rep = (labels[None, :] * (1.0 + rng.normal(0.0, 4.0, (spectra, nl)) * 1e-6)).astype(np.float32)
        keep = rng.random((spectra, nl)) < 0.9
        mz[:, :nl] = np.where(keep, rep, mz[:, :nl])
        it = rng.lognormal(7.0, 1.5, n).astype(np.float32).reshape(spectra, peaks)
        mz.sort(axis=1)  # (m/z ascending, as in an mzML file; intensities are i.i.d., so unpaired order is irrelevant)
        off = np.arange(spectra + 1, dtype=np.uint64) * np.uint64(peaks)
        out.append(RawBatch.from_arrays([""] * spectra, off, mz.reshape(-1), it.reshape(-1), np.full(spectra, 600.0, np.float32),
                                        rng.integers(2, 4, spectra).astype(np.uint8), np.full(spectra, np.nan, np.float32),
                                        np.full(spectra, np.nan, np.float32), np.zeros(spectra, np.float32),
                                        np.full(spectra, np.nan, np.float32), np.full(spectra, f, np.uint32)))
    return out


def measure(batches, iso, level, steps, **kw):
    tmt(batches, iso, level, **kw)  # warm-up
    runs = []
    for _ in range(steps):
        t0 = time.time()
        r = tmt(batches, iso, level, **kw)
        runs.append(dict(r.stage_ms, wall_ms=(time.time() - t0) * 1e3))
    return {k: float(np.median([x[k] for x in runs])) for k in runs[0]}, runs, r


def cpu_slice(batch, labels, level, n=200):
    import tmt_reference as R
    from sage_amd.api import SpectrumProcessor
    proc = SpectrumProcessor(150, True, float(R.min_deisotope_mz(labels)))
    t0 = time.time()
    for i in range(n):
        s = batch.spectrum(i)
        if level == 2:
            p = proc.process(s)
            R.quantify_spectrum(2, np.asarray(p.masses, np.float32), np.asarray(p.intensities, np.float32), labels)
        else:
            m, it, pos = R.process_other_level(s.mz, s.intensity)
            R.quantify_spectrum(3, m, it, labels, raw_position=pos)
    return (time.time() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=12)
    ap.add_argument("--spectra", type=int, default=40000)
    ap.add_argument("--peaks", type=int, default=500)
    ap.add_argument("--ms2-peaks", type=int, default=400)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    iso = Isobaric("Tmt18")
    labels = iso.reporter_masses()
    out = {"workload": {"files": a.files, "spectra_per_file": a.spectra, "labels": len(labels), "ms3_peaks_per_spectrum": a.peaks,
                        "ms2_peaks_per_spectrum": a.ms2_peaks, "ms3_peaks": a.files * a.spectra * a.peaks,
                        "ms2_peaks": a.files * a.spectra * a.ms2_peaks}}
    t0 = time.time()
    ms3 = workload(a.files, a.spectra, a.peaks, labels, seed=1)
    out["generate_s"] = time.time() - t0
    med, runs, r = measure(ms3, iso, 3, a.steps)
    out["level3"] = {"median_ms": med, "runs": runs, "reporters_found": int((r.peak_index >= 0).sum())}
    if not a.no_cpu:
        out["level3"]["cpu_ms_per_spectrum"] = cpu_slice(ms3[0], labels, 3)
    del ms3, r
    ms2 = workload(a.files, a.spectra, a.ms2_peaks, labels, seed=2)
    med, runs, r = measure(ms2, iso, 2, a.steps, take_top_n=150, deisotope=True, min_deisotope_mz=iso.min_deisotope_mz())
    out["level2"] = {"median_ms": med, "runs": runs, "reporters_found": int((r.peak_index >= 0).sum())}
    if not a.no_cpu:
        out["level2"]["cpu_ms_per_spectrum"] = cpu_slice(ms2[0], labels, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
