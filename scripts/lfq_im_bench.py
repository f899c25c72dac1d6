#!/usr/bin/env python3
"""Label-free quantification with an ion-mobility column (sage_hip_lfq_im) at the size of scripts/lfq_bench.py — N files x S MS1
spectra x P peaks, Q quantified peptides — once without and once with a mobility value per peak, and, with --parent-lib, the
no-mobility call of another build of the library (the parent commit's) alternating with this one in the same process.

    python scripts/lfq_im_bench.py [--files 10 --ms1 6000 --peaks 4000 --peptides 40000 --steps 3]
                                   [--parent-lib PATH --rounds 2] [--only plain|im] [--out profiles/lfq_im_bench.json]

Every configuration: one warm-up call, then `steps` timed calls; the stage times are the library's own HIP events, the wall time
is the whole api call.  The mobility column: every peptide has a mobility k0 in [0.6, 1.4] (its feature's ims); an MS1 peak
within 15 ppm of a peptide's charge x isotope m/z gets the k0 of the nearest such peptide * (1 +- 0.8 %), inside that peptide's
default 1 % window, every other peak a uniform value in [0.5, 1.6].  At this density (360 000 theoretical m/z) nearly every peak
has such a neighbour, so a peak passes the window of the nearest peptide and fails most of the other windows that hold its mass:
the run with mobility keeps fewer (peak, window) matches and fewer grids, and the JSON says how many.
Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from lfq_bench import NEUTRON, PROTON, workload  # noqa: E402
from sage_amd import _lib as L  # noqa: E402
from sage_amd.api import LfqSettings, RawBatch, lfq  # noqa: E402


def open_library(path):
    """Point sage_amd at the library at `path` for the LFQ calls.  Another build (the parent commit's) has no sage_hip_lfq_im:
    only the symbols this script calls are bound."""
    lib = C.CDLL(path)
    lib.sage_hip_last_error.restype = C.c_char_p
    lib.sage_hip_lfq.restype = C.c_int
    lib.sage_hip_lfq.argtypes = [C.c_int, C.POINTER(L.SageLfqInput), C.POINTER(L.SageLfqOutput)]
    if hasattr(lib, "sage_hip_lfq_im"):
        lib.sage_hip_lfq_im.restype = C.c_int
        lib.sage_hip_lfq_im.argtypes = [C.c_int, C.POINTER(L.SageLfqInput), C.POINTER(L.SageLfqMobility), C.POINTER(L.SageLfqOutput)]
    L._lib = lib
    return lib


def add_mobility(f, batches, seed=1, spread_pct=0.8, ppm=15.0):
    """f["ims"] and a per-peak mobility column for every batch (see the module docstring); returns the batches with the column"""
    rng = np.random.default_rng(seed)
    mass = f["calcmass"].astype(np.float64)
    k0 = rng.uniform(0.6, 1.4, len(mass)).astype(np.float32)
    f["ims"] = k0
    table = ((mass[:, None, None] + np.arange(3)[None, None, :] * NEUTRON) / np.array([2.0, 3.0, 4.0])[None, :, None] + PROTON).reshape(-1)
    owner = np.repeat(np.arange(len(mass)), 9)
    order = np.argsort(table)
    table, owner = table[order], owner[order]
    out, signal = [], 0
    for b in batches:
        mz = b.mz.astype(np.float64)
        mob = rng.uniform(0.5, 1.6, len(mz)).astype(np.float32)
        j = np.clip(np.searchsorted(table, mz), 1, len(table) - 1)
        j = np.where(np.abs(table[j - 1] - mz) < np.abs(table[j] - mz), j - 1, j)
        hit = np.abs(table[j] - mz) <= ppm * 1e-6 * mz
        mob[hit] = k0[owner[j[hit]]] * (1.0 + rng.uniform(-spread_pct, spread_pct, int(hit.sum())) / 100.0).astype(np.float32)
        signal += int(hit.sum())
        out.append(RawBatch.from_arrays(b.ids, b.peak_off, b.mz, b.intensities, b.precursor_mz, b.precursor_charge, b.isolation_lo,
                                        b.isolation_hi, b.scan_start_time, b.inverse_ion_mobility, b.file_id, mobility=mob))
    return out, signal


def note(msg):
    print(f"[lfq_im_bench] {msg}", file=sys.stderr, flush=True)


def measure(args, batches, steps, ion_mobility, label=""):
    note(f"measuring {label or ('with' if ion_mobility else 'without') + ' mobility'}")
    f, art, pq, al, carbon, sulfur = args
    st = LfqSettings()
    res = lfq(f, None, art, pq, al, batches, carbon, sulfur, st, (2, 4), ion_mobility=ion_mobility)  # warm-up
    runs = []
    for _ in range(steps):
        t0 = time.time()
        res = lfq(f, None, art, pq, al, batches, carbon, sulfur, st, (2, 4), ion_mobility=ion_mobility)
        runs.append(dict(res.stage_ms, wall_ms=(time.time() - t0) * 1e3))
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    return {"median_ms": med, "runs": runs, "contributions": res.n_contributions, "grids": len(res.peptide_idx),
            "peaks_found": int(res.has_peak.sum()), "passing": res.passing, "windows": res.n_windows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=10)
    ap.add_argument("--ms1", type=int, default=6000)
    ap.add_argument("--peaks", type=int, default=4000)
    ap.add_argument("--peptides", type=int, default=40000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another build of libsage_hip.so: its sage_hip_lfq alternates with this one's")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=("plain", "im"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t0 = time.time()
    f, art, pq, al, batches, carbon, sulfur = workload(a.files, a.ms1, a.peaks, a.peptides)
    args = (f, art, pq, al, carbon, sulfur)
    note(f"workload generated in {time.time() - t0:.0f} s")
    this_lib = L.lib_path()
    L.load()  # (builds the library when it is missing)
    out = {"workload": {"files": a.files, "ms1_per_file": a.ms1, "peaks_per_spectrum": a.peaks, "peptides": a.peptides,
                        "ms1_peaks": a.files * a.ms1 * a.peaks}, "steps": a.steps}
    if a.only != "im":
        order = []
        for r in range(a.rounds if a.parent_lib else 1):
            if a.parent_lib:
                open_library(a.parent_lib)
                order.append(("parent", measure(args, batches, a.steps, False, f"parent build, round {r}")))
            open_library(this_lib)
            order.append(("this", measure(args, batches, a.steps, False, f"this build, round {r}")))
        out["no_mobility"] = [dict(build=k, **v) for k, v in order]
        mine = [r for k, v in order if k == "this" for r in v["runs"]]
        out["no_mobility_this_median_ms"] = {k: float(np.median([r[k] for r in mine])) for k in mine[0]}
        if a.parent_lib:
            theirs = [r for k, v in order if k == "parent" for r in v["runs"]]
            cmp = {}
            for k in ("trace_ms", "device_ms", "wall_ms"):
                p = [r[k] for r in theirs]
                rounds = [v["median_ms"][k] for kk, v in order if kk == "parent"]
                cmp[k] = {"parent_median": float(np.median(p)), "parent_min": min(p), "parent_max": max(p),
                          "parent_round_medians": rounds, "this_median": out["no_mobility_this_median_ms"][k],
                          "this_minus_parent": out["no_mobility_this_median_ms"][k] - float(np.median(p)),
                          "parent_spread": max(p) - min(p)}
                cmp[k]["within_parent_spread"] = cmp[k]["this_minus_parent"] <= cmp[k]["parent_spread"]
            out["parent_comparison"] = cmp
    if a.only != "plain":
        open_library(this_lib)
        t1 = time.time()
        with_mob, signal = add_mobility(f, batches)
        out["mobility_column"] = {"generate_s": time.time() - t1, "signal_peaks": signal}
        out["with_mobility"] = measure(args, with_mob, a.steps, True)
        if "no_mobility_this_median_ms" in out:
            base, im = out["no_mobility_this_median_ms"], out["with_mobility"]["median_ms"]
            out["mobility_cost_ms"] = {k: im[k] - base[k] for k in base}
            out["mobility_cost_pct"] = {k: 100.0 * (im[k] - base[k]) / base[k] for k in base if base[k] > 0}
    out["total_s"] = time.time() - t0
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
