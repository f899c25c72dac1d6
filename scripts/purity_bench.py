"""Precursor purity at scale: sage_hip_precursor_purity on a world of the label-free benchmark's shape,

    10 files x 6 000 MS1 scans x 4 000 peaks, 500 000 queries

every spectrum sorted by m/z; a query's precursor is a peak of its spectrum, charges 2..4, the default isolation window.

    python scripts/purity_bench.py [--out profiles/purity_bench.json] [--small]

Times: the call's HIP-event times (upload_ms, kernel_ms, device_ms) as the median of three calls after one warm-up call, for the
routes the flags choose (every spectrum sorted) and again with SAGE_HIP_PURITY_SCAN=1 (every spectrum scanned through LDS); beside them
the wall time of ONE host thread running the same arithmetic on the same world (sage_amd/csrc/purity.h through
tests/hostemu/purity_emu.cpp, g++ -O2), whose results the device's must equal bit for bit on both routes — the script checks that.
The sorted route's kernel time stands beside the time HBM needs for the bytes that route asks for.  No threshold: the figures are
what they are.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sage_amd.api import RawBatch, device_count, precursor_purity  # noqa: E402

HBM_BYTES_PER_S = 6.3e12  # what a streaming kernel reaches on one MI355X (8 TB/s on paper)
FIELDS = ("n_window", "n_matched", "total", "matched", "below", "purity")


def world(n_files, n_ms1, n_peaks, n_queries, seed):
    rng = np.random.default_rng(seed)
    batches = []
    for f in range(n_files):
        mz = np.sort(rng.uniform(300.0, 1600.0, (n_ms1, n_peaks)).astype(np.float32), axis=1).reshape(-1)
        it = rng.lognormal(8.0, 1.5, n_ms1 * n_peaks).astype(np.float32)
        nan = np.full(n_ms1, np.nan, np.float32)
        batches.append(RawBatch.from_arrays([""] * n_ms1, np.arange(n_ms1 + 1, dtype=np.uint64) * np.uint64(n_peaks), mz, it, np.zeros(n_ms1),
                                            np.zeros(n_ms1, np.uint8), nan, nan, np.arange(n_ms1), nan, np.full(n_ms1, f, np.uint32)))
    index = rng.integers(0, n_files * n_ms1, n_queries).astype(np.uint64)
    peak = rng.integers(0, n_peaks, n_queries)
    mz = np.array([batches[int(s) // n_ms1].mz[(int(s) % n_ms1) * n_peaks + int(p)] for s, p in zip(index, peak)], np.float32)
    return batches, index, mz, rng.integers(2, 5, n_queries).astype(np.uint8)


def host_emulation(tmp):
    lib = os.path.join(tmp, "libpurity_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "hostemu", "purity_emu.cpp"), "-o", lib])
    emu = C.CDLL(lib)
    fp, dp, up, u8p, u64p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_uint32, C.c_uint8, C.c_uint64))
    emu.emu_purity.argtypes = [C.c_uint64, u64p, fp, fp, C.c_uint64, u64p, fp, u8p, fp, fp, C.c_float, C.c_float, C.c_float, C.c_uint32,
                               up, up, dp, dp, dp, fp]
    emu.emu_purity.restype = C.c_int

    def run(batches, index, mz, charge):
        off = np.concatenate([[0]] + [b.peak_off[1:] + np.uint64(sum(int(a.peak_off[-1]) for a in batches[:k])) for k, b in enumerate(batches)])
        off = np.ascontiguousarray(off, np.uint64)
        pm, pi = np.concatenate([b.mz for b in batches]), np.concatenate([b.intensities for b in batches])
        n = len(index)
        out = {"n_window": np.zeros(n, np.uint32), "n_matched": np.zeros(n, np.uint32), "total": np.zeros(n), "matched": np.zeros(n),
               "below": np.zeros(n), "purity": np.zeros(n, np.float32)}
        ptr = lambda a, t: a.ctypes.data_as(t)
        t = time.time()
        rc = emu.emu_purity(len(off) - 1, ptr(off, u64p), ptr(pm, fp), ptr(pi, fp), n, ptr(index, u64p), ptr(mz, fp), ptr(charge, u8p), None, None,
                            10.0, -0.5, 0.5, 4, ptr(out["n_window"], up), ptr(out["n_matched"], up), ptr(out["total"], dp),
                            ptr(out["matched"], dp), ptr(out["below"], dp), ptr(out["purity"], fp))
        wall = (time.time() - t) * 1e3
        assert rc == 0, rc
        return wall, out
    return run


def timed(batches, index, mz, charge):
    t = time.time()
    first = precursor_purity(batches, index, mz, charge)  # warm-up: code objects loaded
    first_wall = (time.time() - t) * 1e3
    runs, walls = [], []
    for _ in range(3):
        t = time.time()
        r = precursor_purity(batches, index, mz, charge)
        walls.append((time.time() - t) * 1e3)
        runs.append(r.stage_ms)
        assert all(getattr(r, k).tobytes() == getattr(first, k).tobytes() for k in FIELDS), "the call is not repeatable"
    med = {key: float(np.median([s[key] for s in runs])) for key in runs[0]}
    return first, {**med, "stage_ms_runs": runs, "call_wall_ms": float(np.median(walls)), "first_call_wall_ms": first_wall,
                   "n_sorted_spectra": first.n_sorted_spectra, "n_scanned_spectra": first.n_scanned_spectra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "purity_bench.json"))
    ap.add_argument("--small", action="store_true", help="a tenth of the scans and queries (a quick look, not the committed figures)")
    args = ap.parse_args()
    if device_count() <= 0:
        raise SystemExit("purity_bench: no HIP device visible (there is no CPU fallback, and a CPU time would say nothing)")
    n_files, n_ms1, n_peaks, n_queries = 10, 6000, 4000, 500000
    if args.small:
        n_ms1, n_queries = n_ms1 // 10, n_queries // 10
    batches, index, mz, charge = world(n_files, n_ms1, n_peaks, n_queries, 23)
    os.environ.pop("SAGE_HIP_PURITY_SCAN", None)
    chosen, chosen_times = timed(batches, index, mz, charge)
    os.environ["SAGE_HIP_PURITY_SCAN"] = "1"  # (read once per call)
    scanned, scanned_times = timed(batches, index, mz, charge)
    os.environ.pop("SAGE_HIP_PURITY_SCAN")
    with tempfile.TemporaryDirectory() as tmp:
        host_ms, host = host_emulation(tmp)(batches, index, mz, charge)
    same = all(host[k].tobytes() == getattr(chosen, k).tobytes() == getattr(scanned, k).tobytes() for k in FIELDS)
    assert same, "the device (either route) and the host emulation differ"
    # what the sorted route asks memory for, per query: 2 intervals x (a 64-ary search over the spectrum: one round of 64 probes 4 B
    # each, every probe in a line of its own, then 64 contiguous m/z; the end next to the first: 64 contiguous m/z) + 8 B per peak of
    # the window and of the `below` interval.  Requested bytes count 4 B per probe, line bytes 64 B per probe.  kernel_ms also holds
    # the flag pass, which reads the m/z of every queried spectrum once (flag_pass_bytes_inside_kernel_ms).
    searches = 2 * n_queries
    window_bytes = 8 * int(chosen.n_window.sum())
    requested = searches * (64 * 4 + 2 * 256) + window_bytes
    lines = searches * (64 * 64 + 2 * 256) + window_bytes
    spectra_once = 8 * n_peaks * len(np.unique(index))
    k_ms = chosen_times["kernel_ms"]
    out = {"timing": "HIP events of the call (upload_ms, kernel_ms, device_ms): median of 3 calls after one warm-up call; "
                     "host_emulation_wall_ms: one thread, one run, host clock",
           "world": {"files": n_files, "ms1_per_file": n_ms1, "peaks_per_spectrum": n_peaks, "queries": n_queries,
                     "ms1_bytes": 8 * n_files * n_ms1 * n_peaks, "spectra_with_a_query": int(len(np.unique(index))),
                     "mean_peaks_in_window": float(chosen.n_window.mean()), "mean_purity": float(chosen.purity.mean())},
           "routes_as_flagged": chosen_times, "scan_route_forced": scanned_times, "host_emulation_wall_ms": host_ms,
           "device_equals_host_emulation_bit_for_bit_on_both_routes": bool(same),
           "sorted_route_bytes": {"requested_bytes": requested, "cache_line_bytes": lines, "every_queried_spectrum_once_bytes": spectra_once,
                                  "flag_pass_bytes_inside_kernel_ms": spectra_once // 2,
                                  "hbm_bytes_per_s": HBM_BYTES_PER_S, "hbm_ms_for_requested": requested / HBM_BYTES_PER_S * 1e3,
                                  "hbm_ms_for_cache_lines": lines / HBM_BYTES_PER_S * 1e3,
                                  "kernel_ms_over_hbm_ms_for_requested": k_ms / (requested / HBM_BYTES_PER_S * 1e3),
                                  "kernel_ms_over_hbm_ms_for_cache_lines": k_ms / (lines / HBM_BYTES_PER_S * 1e3)}}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=2)
        fh.write("\n")


if __name__ == "__main__":
    main()
