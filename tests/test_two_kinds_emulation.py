"""CPU tests of the two-kind forms of the kind walks (sage_amd/csrc/core.h: kinds2_bound / kinds2_nt_mask / kinds2_idx0_c /
kinds2_decode), compiled for the host (tests/hostemu/two_kinds_emu.cpp): what the KINDS2 instances of kernels.hip: score_candidates
— a database of two ion kinds, the first n-terminal — use instead of the kind_seg_first / kind_seg_next walk of a chunk's segments
and the `while (idx >= lm1)` decode of an ion.  For every lm1 from 1 to 200 and every chunk start j0 in {0, 64, 128, ...} below
2 * lm1: the segments, the n-terminal mask, the idx0 handed to run_matched_mask and the kind and index of every ion are the general
walk's; and the counts and runs the cooperative path derives from hit masks are the same both ways."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "two_kinds_emu.cpp")
LIB = os.path.join(HERE, "hostemu", "libtwo_kinds_emu.so")
u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "..", "sage_amd", "csrc", "core.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.emu_two_kinds.restype, lib.emu_two_kinds.argtypes = C.c_uint64, [C.c_uint32, u64p]
    lib.emu_two_kinds_counts.restype = None
    lib.emu_two_kinds_counts.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    return lib


def test_segments_masks_and_every_ion(emu):
    """lm1 1 .. 200 x every chunk: boundary, masks, idx0 and the (kind, index) of every ion against the general walks"""
    bad = np.zeros(3, np.uint64)
    for lm1 in range(1, 201):
        n = emu.emu_two_kinds(lm1, bad.ctypes.data_as(u64p))
        assert n == 2 * lm1, (lm1, [int(v) for v in bad])


def test_counts_and_runs_from_hit_masks(emu):
    """random hit masks inside the candidate's ions — sparse, dense, full, one side of the boundary only — at one to three charges,
    fresh and carried states: the packed counts and both Run states of the general walk and of the two-kind form, every field"""
    rng = np.random.default_rng(14)
    out = np.zeros(6, np.uint32)
    cases = one_sided = both_sides = 0
    for lm1 in list(range(1, 72)) + [100, 127, 128, 129, 200]:
        nions = 2 * lm1
        for j0 in range(0, nions, 64):
            n_here = min(64, nions - j0)
            in_chunk = (1 << n_here) - 1
            bound = min(max(lm1 - j0, 0), 64)
            nt = (1 << bound) - 1
            for rep in range(24):
                ks = []
                for _ in range(3):
                    k = int(rng.integers(0, 1 << 63, dtype=np.uint64)) << 1 | int(rng.integers(0, 2))
                    mode = rep % 6
                    if mode == 0:
                        k &= int(rng.integers(0, 1 << 63, dtype=np.uint64)) << 1
                    elif mode == 1:
                        k = (1 << 64) - 1
                    elif mode == 2:
                        k &= nt  # kind 0 only
                    elif mode == 3:
                        k &= ~nt  # kind 1 only
                    ks.append(k & in_chunk)
                if rep % 5 == 4:
                    ks[2] = 0
                any_k = ks[0] | ks[1] | ks[2]
                one_sided += bool(any_k) and (not (any_k & nt) or not (any_k & ~nt & in_chunk))
                both_sides += bool(any_k & nt) and bool(any_k & ~nt & in_chunk)
                # carried states: fresh, or what an earlier chunk of the same series left right in front of this one
                mm = int(rng.integers(0, 40)) | int(rng.integers(0, 40)) << 16
                b_run = y_run = 0
                if rep % 2 and j0:
                    nxt = min(j0, lm1)
                    b_run = nxt | 3 << 10 | 5 << 20
                    y_run = max(j0 - lm1, 0) | 2 << 10 | 2 << 20
                emu.emu_two_kinds_counts(lm1, j0, ks[0], ks[1], ks[2], mm, b_run, y_run, out.ctypes.data_as(u32p))
                assert tuple(out[:3]) == tuple(out[3:]), (lm1, j0, [hex(k) for k in ks], mm, b_run, y_run, out.tolist())
                cases += 1
    assert cases > 3000 and one_sided > 500 and both_sides > 500, (cases, one_sided, both_sides)
