"""CPU tests of the mask forms of Run (sage_amd/csrc/core.h: run_matched_mask for both packed widths, kind_seg_first /
kind_seg_next / kind_seg_mask), compiled for the host (tests/hostemu/run_mask_emu.cpp): what the cooperative path of kernels.hip:
score_candidates takes a heavy candidate's longest runs and kind segments from.  run_matched_mask(r, S, idx0) must leave exactly
what run_matched_packed(r, idx0 + t) for every set bit t of S in ascending order leaves — every field, both widths —, whether a
bit is offered once or once per fragment charge; the segments must be the `while (idx >= lm1)` walk's (kind, index) of every ion."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "run_mask_emu.cpp")
LIB = os.path.join(HERE, "hostemu", "librun_mask_emu.so")
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "..", "sage_amd", "csrc", "core.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.emu_run_mask32.restype, lib.emu_run_mask32.argtypes = C.c_uint32, [C.c_uint32, C.c_uint64, C.c_uint32]
    lib.emu_run_mask64.restype, lib.emu_run_mask64.argtypes = C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint32]
    lib.emu_run_seq32.restype, lib.emu_run_seq32.argtypes = C.c_uint32, [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.emu_run_seq64.restype, lib.emu_run_seq64.argtypes = C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.emu_run_mask_exhaustive.restype, lib.emu_run_mask_exhaustive.argtypes = C.c_uint64, [C.c_uint32, u64p]
    lib.emu_run_mask_random.restype, lib.emu_run_mask_random.argtypes = C.c_uint64, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, u64p]
    lib.emu_kind_segments.restype, lib.emu_kind_segments.argtypes = C.c_uint64, [C.c_uint32, C.c_uint32, u64p]
    return lib


def fields(r, wide):
    bits = 21 if wide else 10
    m = (1 << bits) - 1
    return dict(next=r & m, length=(r >> bits) & m, longest=r >> (2 * bits))


def describe(bad, wide):
    r, s, idx0, got, want = (int(v) for v in bad)
    return f"state {fields(r, wide)}, S = {s:#x}, idx0 = {idx0}: mask form {fields(got, wide)}, sequential {fields(want, wide)}"


@pytest.mark.parametrize("wide", [0, 1])
def test_the_reference_quirks_by_hand(emu, wide):
    mask, seq = (emu.emu_run_mask64, emu.emu_run_seq64) if wide else (emu.emu_run_mask32, emu.emu_run_seq32)
    bits = 21 if wide else 10

    def st(nxt, length, longest):
        return nxt | (length << bits) | (longest << (2 * bits))
    # an empty mask leaves the state alone
    assert mask(st(5, 2, 3), 0, 7) == st(5, 2, 3)
    # a fresh Run ignores a first match at index 0 (the reference's `last == index` with last = 0): nothing changes ...
    assert mask(0, 1, 0) == 0
    # ... and the run behind it starts at index 1
    assert mask(0, 0b111, 0) == st(3, 2, 2)
    # the same bits one index further on: a run of three
    assert mask(0, 0b111, 1) == st(4, 3, 3)
    # a run that continues across a seam: next == the first index
    assert mask(st(64, 4, 4), 0b11, 64) == st(66, 6, 6)
    # `last` carried in on the first bit (an ion matched again at another charge, or by the next kind of the series): ignored, and
    # the run goes on behind it
    assert mask(st(8, 2, 5), 0b11, 7) == st(9, 3, 5)
    # a gap: the carried run ends, longest keeps the maximum of the carried value and the runs of the mask
    assert mask(st(3, 3, 3), 0b0111_1011_0000, 0) == st(11, 4, 4)
    # bit 63 and a full mask
    assert mask(0, (1 << 64) - 1, 100) == st(164, 64, 64)
    assert mask(st(100, 7, 9), 1 << 63, 37) == st(101, 8, 9)
    for r, s, idx0 in ((0, 0b1011, 0), (st(8, 2, 5), 0xF0F1, 7), (st(3, 1, 5), 0xFFFF_0000_FFFF_0001, 2)):
        for times in (1, 2, 3):
            assert mask(r, s, idx0) == seq(r, s, idx0, times), (r, s, idx0, times)


@pytest.mark.parametrize("wide", [0, 1])
def test_every_mask_below_2_16(emu, wide):
    """every S below 2^16 x idx0 in {0, 1, 2, 7} x the fresh state and next in {idx0 - 1 .. idx0 + 2, idx0 + 5} x length 1 / 3 x
    longest = length / length + 4"""
    bad = np.zeros(5, np.uint64)
    n = emu.emu_run_mask_exhaustive(wide, bad.ctypes.data_as(u64p))
    assert n, describe(bad, wide)
    # idx0 = 0: four carried values of next, the others five, two lengths and two longests each, and the fresh state
    assert n == (1 + 4 * 4 + 3 * (1 + 5 * 4)) * (1 << 16)


@pytest.mark.parametrize("wide,max_idx0", [(0, 1022 - 63), (1, 1022 - 63), (1, 65535 - 63), (1, (1 << 21) - 2 - 63)])
def test_random_64_bit_masks(emu, wide, max_idx0):
    """64-bit masks with bit 63 and full masks among them, ion indices up to 1022 in the one-register form and beyond 1023 in the
    wide one, every bit offered one to three times, carried states from earlier chunks and earlier kinds"""
    bad = np.zeros(5, np.uint64)
    n = emu.emu_run_mask_random(wide, 1000 + max_idx0, 400_000, max_idx0, bad.ctypes.data_as(u64p))
    assert n == 400_000, describe(bad, wide)


def test_kind_segments(emu):
    """lm1 1 .. 70 x n_kinds 1 .. 8 x every chunk against the subtract loop"""
    bad = np.zeros(3, np.uint64)
    for lm1 in range(1, 71):
        for n_kinds in range(1, 9):
            n = emu.emu_kind_segments(lm1, n_kinds, bad.ctypes.data_as(u64p))
            assert n == lm1 * n_kinds, (lm1, n_kinds, [int(v) for v in bad])
