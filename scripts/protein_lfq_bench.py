"""The protein roll-up of label-free quantification at scale (MaxLFQ): sage_hip_protein_lfq on two synthetic worlds,

    10 000 proteins x  20 files        4 000 proteins x 200 files

rows per protein geometric with mean 8 and one protein of 3 000 rows, 35 % of the values missing.

    python scripts/protein_lfq_bench.py [--out profiles/protein_lfq_bench.json] [--small]

Times: the call's HIP-event stage times (logarithms and grouping, pair medians, solves, the whole call with its copies) as the median
of three calls after one warm-up call; beside them the wall time of ONE thread of the host running the same arithmetic on the same
world (sage_amd/csrc/maxlfq.h through tests/hostemu/maxlfq_emu.cpp, g++ -O2), whose results the device's must equal bit for bit —
the script checks that.  No threshold: the figures are what they are.
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

from sage_amd.api import device_count, protein_lfq  # noqa: E402

WORLDS = (("10000x20", 10000, 20), ("4000x200", 4000, 200))


def world(n_proteins, n_files, seed):
    rng = np.random.default_rng(seed)
    rows = rng.geometric(1.0 / 8.0, n_proteins)
    rows[n_proteins // 2] = 3000
    protein = np.repeat(np.arange(n_proteins, dtype=np.uint32), rows)
    rng.shuffle(protein)
    level = rng.normal(16.0, 2.0, n_proteins)[protein][:, None] + rng.normal(0.0, 0.5, (1, n_files))
    areas = np.exp(level + rng.normal(0.0, 0.3, (len(protein), n_files)))
    areas[rng.random(areas.shape) < 0.35] = 0.0
    return areas, protein


def host_emulation(tmp):
    lib = os.path.join(tmp, "libmaxlfq_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "hostemu", "maxlfq_emu.cpp"), "-o", lib])
    emu = C.CDLL(lib)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    emu.emu_protein_lfq.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, dp, up, dp, dp, up, up, up, dp, up]
    emu.emu_protein_lfq.restype = C.c_int

    def run(areas, protein, n_proteins):
        n = areas.shape[1]
        la, inten = np.zeros((n_proteins, n)), np.zeros((n_proteins, n))
        comp, used, ncomp = np.zeros((n_proteins, n), np.uint32), np.zeros(n_proteins, np.uint32), np.zeros(n_proteins, np.uint32)
        t = time.time()
        rc = emu.emu_protein_lfq(len(areas), n, n_proteins, 1, areas.ctypes.data_as(dp), protein.ctypes.data_as(up), la.ctypes.data_as(dp),
                                 inten.ctypes.data_as(dp), comp.ctypes.data_as(up), used.ctypes.data_as(up), ncomp.ctypes.data_as(up), None, None)
        wall = (time.time() - t) * 1e3
        assert rc == 0, rc
        return wall, la, inten, comp
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "protein_lfq_bench.json"))
    ap.add_argument("--small", action="store_true", help="a tenth of the proteins (a quick look, not the committed figures)")
    args = ap.parse_args()
    if device_count() <= 0:
        raise SystemExit("protein_lfq_bench: no HIP device visible (there is no CPU fallback, and a CPU time would say nothing)")
    out = {"timing": "HIP events of the call (log_ms, median_ms, solve_ms, device_ms): median of 3 calls after one warm-up call; "
                     "host_emulation_wall_ms: one thread, one run, host clock", "worlds": {}}
    with tempfile.TemporaryDirectory() as tmp:
        emulate = host_emulation(tmp)
        for k, (name, n_proteins, n_files) in enumerate(WORLDS):
            if args.small:
                n_proteins //= 10
            areas, protein = world(n_proteins, n_files, 17 + k)
            t = time.time()
            first = protein_lfq(areas, protein, n_proteins)  # warm-up: code objects loaded
            first_wall = (time.time() - t) * 1e3
            runs, walls = [], []
            for _ in range(3):
                t = time.time()
                r = protein_lfq(areas, protein, n_proteins)
                walls.append((time.time() - t) * 1e3)
                runs.append(r.stage_ms)
                assert r.log_abundance.tobytes() == first.log_abundance.tobytes(), "the call is not repeatable"
            host_ms, la, inten, comp = emulate(areas, protein, n_proteins)
            same = (la.tobytes() == first.log_abundance.tobytes() and inten.tobytes() == first.intensity.tobytes() and
                    comp.tobytes() == first.component.tobytes())
            assert same, "the device and the host emulation differ"
            med = {key: float(np.median([s[key] for s in runs])) for key in runs[0]}
            out["worlds"][name] = {
                "proteins": n_proteins, "files": n_files, "rows": int(len(protein)), "largest_protein_rows": 3000,
                "pairs_per_protein": n_files * (n_files - 1) // 2, "missing": 0.35, "n_batches": int(first.n_batches),
                **med, "stage_ms_runs": runs, "call_wall_ms": float(np.median(walls)), "first_call_wall_ms": first_wall,
                "host_emulation_wall_ms": host_ms, "device_equals_host_emulation_bit_for_bit": bool(same),
                "quantified_cells": int((~np.isnan(first.log_abundance)).sum()),
                "proteins_with_more_than_one_component": int((first.n_components > 1).sum()),
            }
            print(name, json.dumps(out["worlds"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=2)
        fh.write("\n")


if __name__ == "__main__":
    main()
