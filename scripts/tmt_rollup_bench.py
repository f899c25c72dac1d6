"""The roll-up of TMT reporter intensities at scale: sage_hip_tmt_rollup on

    1 000 000 rows x 18 channels in 10 000 groups         (both summaries, both normalisations)
    one group of 100 000 rows x 18 channels               (Median: the route over the group's columns in global memory)

rows per group uneven (a gamma-distributed share), 10 % of the cells missing, 2 % of the rows ignored.

    python scripts/tmt_rollup_bench.py [--out profiles/tmt_rollup_bench.json] [--small]

Times: the call's HIP-event stage times (norm_ms, summary_ms, device_ms) and its wall time as the median of three calls after one
warm-up call.  For scale, on the same input: one thread of the host running the same arithmetic (sage_amd/csrc/tmt_rollup.h through
tests/hostemu/tmt_rollup_emu.cpp, g++ -O2), whose results the device's must equal bit for bit — the script checks that; a vectorised
numpy reading of the contract (not bit-exact: numpy's own sums and logarithm); and the plain-Python restatement
(tests/tmt_rollup_reference.py) on the first 10 000 rows only — at 18 million cells its `decimal` logarithms would take hours.  No
threshold: the figures are what they are.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sage_amd.api import device_count, tmt_rollup  # noqa: E402

NONE = 0xFFFFFFFF
CODE = {"None": 0, "Total": 1, "Sum": 0, "Median": 1}
PAIRS = [(s, n) for s in ("Sum", "Median") for n in ("Total", "None")]


def world(n_rows, n_labels, n_groups, seed):
    rng = np.random.default_rng(seed)
    share = rng.gamma(2.0, 1.0, n_groups)
    group = rng.choice(n_groups, n_rows, p=share / share.sum()).astype(np.uint32)
    level = rng.normal(10.0, 1.5, n_groups)[group][:, None] + rng.normal(0.0, 0.4, (1, n_labels))
    x = np.exp(level + rng.normal(0.0, 0.3, (n_rows, n_labels))).astype(np.float32)
    x[rng.random(x.shape) < 0.10] = 0.0
    group[rng.random(n_rows) < 0.02] = NONE
    return x, group


def host_emulation(tmp):
    lib = os.path.join(tmp, "libtmt_rollup_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "hostemu", "tmt_rollup_emu.cpp"), "-o", lib])
    emu = C.CDLL(lib)
    dp, up, fp = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    emu.emu_tmt_rollup.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, fp, up, dp, dp, up, up, dp, dp,
                                   C.POINTER(C.c_uint64)]
    emu.emu_tmt_rollup.restype = C.c_int

    def run(x, group, n_groups, summary, normalise):
        n = x.shape[1]
        ab, la, nc = np.zeros((n_groups, n)), np.zeros((n_groups, n)), np.zeros((n_groups, n), np.uint32)
        used, f, s, total = np.zeros(n_groups, np.uint32), np.zeros(n), np.zeros(n), C.c_uint64(0)
        t = time.time()
        rc = emu.emu_tmt_rollup(len(x), n, n_groups, 1, CODE[normalise], CODE[summary], x.ctypes.data_as(fp), group.ctypes.data_as(up),
                                ab.ctypes.data_as(dp), la.ctypes.data_as(dp), nc.ctypes.data_as(up), used.ctypes.data_as(up),
                                f.ctypes.data_as(dp), s.ctypes.data_as(dp), C.byref(total))
        wall = (time.time() - t) * 1e3
        assert rc == 0, rc
        return wall, ab, la, nc, used, f, s
    return run


def numpy_reading(x, group, n_groups, summary, normalise):
    """the contract with numpy's own reductions (their order of addition and logarithm are numpy's): wall ms and the abundances"""
    t = time.time()
    v = x.astype(np.float64)
    ok = (v > 0) & (v < np.inf)
    used = (group != NONE) & (ok.sum(axis=1) >= 1)
    ok &= used[:, None]
    S, cells = np.where(ok, v, 0.0).sum(axis=0), ok.sum(axis=0)
    f = np.ones(v.shape[1])
    if normalise == "Total" and (cells > 0).any():
        f[cells > 0] = S[cells > 0].mean() / S[cells > 0]
    w = v * f
    g = group[used].astype(np.int64)
    ab = np.zeros((n_groups, v.shape[1]))
    if summary == "Sum":
        np.add.at(ab, g, np.where(ok, w, 0.0)[used])
    else:
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (nanmedian of a channel without a present cell)
            logs = np.where(ok, np.log(np.where(ok, w, 1.0)), np.nan)[used]
            centre = np.nanmean(logs, axis=1)
            d = logs - centre[:, None]
            order = np.argsort(g, kind="stable")
            bounds = np.searchsorted(g[order], np.arange(n_groups + 1))
            for k in range(n_groups):
                rows = order[bounds[k]:bounds[k + 1]]
                if len(rows):
                    ab[k] = np.exp(np.nanmedian(d[rows], axis=0) + centre[rows].mean())
            ab = np.nan_to_num(ab)
    return (time.time() - t) * 1e3, ab


def measure(x, group, n_groups, summary, normalise, emulate):
    t = time.time()
    first = tmt_rollup(x, group, n_groups, 1, normalise, summary)  # warm-up: code objects loaded
    first_wall = (time.time() - t) * 1e3
    runs, walls = [], []
    for _ in range(3):
        t = time.time()
        r = tmt_rollup(x, group, n_groups, 1, normalise, summary)
        walls.append((time.time() - t) * 1e3)
        runs.append(r.stage_ms)
        assert r.log_abundance.tobytes() == first.log_abundance.tobytes() and r.abundance.tobytes() == first.abundance.tobytes(), \
            "the call is not repeatable"
    host_ms, ab, la, nc, used, f, s = emulate(x, group, n_groups, summary, normalise)
    same = (ab.tobytes() == first.abundance.tobytes() and la.tobytes() == first.log_abundance.tobytes() and
            nc.tobytes() == first.n_cells.tobytes() and used.tobytes() == first.n_rows_used.tobytes() and
            f.tobytes() == first.factor.tobytes() and s.tobytes() == first.column_sum.tobytes())
    assert same, "the device and the host emulation differ"
    numpy_ms, nab = numpy_reading(x, group, n_groups, summary, normalise)
    quantified = first.abundance > 0
    worst = float(np.max(np.abs(nab[quantified] / first.abundance[quantified] - 1.0))) if quantified.any() else 0.0
    med = {key: float(np.median([q[key] for q in runs])) for key in runs[0]}
    return first, {**med, "stage_ms_runs": runs, "call_wall_ms": float(np.median(walls)), "first_call_wall_ms": first_wall,
                   "host_emulation_wall_ms": host_ms, "device_equals_host_emulation_bit_for_bit": bool(same),
                   "numpy_reading_wall_ms": numpy_ms, "numpy_reading_largest_relative_gap": worst,
                   "n_used_rows": first.n_used_rows, "n_long_groups": first.n_long_groups, "n_label_slabs": first.n_label_slabs,
                   "largest_group_rows": int(first.n_rows_used.max()), "quantified_cells": int(quantified.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tmt_rollup_bench.json"))
    ap.add_argument("--small", action="store_true", help="a tenth of the rows and groups (a quick look, not the committed figures)")
    args = ap.parse_args()
    if device_count() <= 0:
        raise SystemExit("tmt_rollup_bench: no HIP device visible (there is no CPU fallback, and a CPU time would say nothing)")
    import tmt_rollup_reference as REF
    scale = 10 if args.small else 1
    n_rows, n_labels, n_groups, long_rows, sample = 1_000_000 // scale, 18, 10_000 // scale, 100_000 // scale, 10_000 // scale
    out = {"timing": "HIP events of the call (norm_ms, summary_ms, device_ms) and its wall time: median of 3 calls after one warm-up "
                     "call; host_emulation_wall_ms / numpy_reading_wall_ms: one thread, one run, host clock; "
                     "python_restatement: the first rows only, one run",
           "workload": {"rows": n_rows, "channels": n_labels, "groups": n_groups, "missing": 0.10, "ignored_rows": 0.02},
           "pairs": {}, "long_group": {}, "python_restatement": {}}
    with tempfile.TemporaryDirectory() as tmp:
        emulate = host_emulation(tmp)
        x, group = world(n_rows, n_labels, n_groups, 23)
        for summary, normalise in PAIRS:
            _, res = measure(x, group, n_groups, summary, normalise, emulate)
            out["pairs"][f"{summary}/{normalise}"] = res
            print(summary, normalise, json.dumps(res), flush=True)
        for summary in ("Sum", "Median"):
            xs, gs = x[:sample].tolist(), group[:sample].tolist()
            t = time.time()
            REF.tmt_rollup(xs, gs, n_groups, 1, "Total", summary, n_labels=n_labels)
            out["python_restatement"][f"{summary}/Total"] = {"rows": sample, "wall_ms": (time.time() - t) * 1e3}
            print("python restatement", summary, json.dumps(out["python_restatement"][f"{summary}/Total"]), flush=True)
        xl, _ = world(long_rows, n_labels, 1, 29)
        gl = np.zeros(long_rows, np.uint32)
        for summary in ("Median", "Sum"):
            first, res = measure(xl, gl, 1, summary, "Total", emulate)
            assert first.n_long_groups == (1 if summary == "Median" else 0)
            out["long_group"][f"{summary}/Total"] = {"rows": long_rows, "channels": n_labels, **res}
            print("long group", summary, json.dumps(out["long_group"][f"{summary}/Total"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=2)
        fh.write("\n")


if __name__ == "__main__":
    main()
