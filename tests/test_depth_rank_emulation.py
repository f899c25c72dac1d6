"""CPU tests of the depth ranks and the min-rank of a tolerance window (sage_amd/csrc/core.h: depth_rank_of,
min_rank_in_window_lockstep), compiled for the host (tests/hostemu/depth_rank_emu.cpp): what the two localisation kernels of
kernels.hip count with, against the plain restatement of tests/localise_reference.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import localise_reference as LR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "depth_rank_emu.cpp")
LIB = os.path.join(HERE, "hostemu", "libdepth_rank_emu.so")
f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
TOL_KINDS = {"ppm": 0, "pct": 1, "da": 2}


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "..", "sage_amd", "csrc", "core.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.emu_depth_ranks.restype, lib.emu_depth_ranks.argtypes = None, [f32p, f32p, C.c_uint32, u8p]
    lib.emu_min_rank.restype = C.c_uint32
    lib.emu_min_rank.argtypes = [f32p, u8p, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float]
    lib.emu_most_intense.restype = C.c_int
    lib.emu_most_intense.argtypes = [f32p, f32p, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float]
    lib.emu_depth_constants.restype, lib.emu_depth_constants.argtypes = C.c_uint32, [C.c_uint32]
    return lib


def ranks_of(emu, masses, intens):
    masses, intens = np.ascontiguousarray(masses, np.float32), np.ascontiguousarray(intens, np.float32)
    out = np.zeros(max(len(masses), 1), np.uint8)
    emu.emu_depth_ranks(masses.ctypes.data_as(f32p), intens.ctypes.data_as(f32p), len(masses), out.ctypes.data_as(u8p))
    return out[:len(masses)]


def min_rank_of(emu, masses, ranks, center, tol):
    masses, ranks = np.ascontiguousarray(masses, np.float32), np.ascontiguousarray(ranks, np.uint8)
    if len(masses) == 0:
        masses, ranks = np.zeros(1, np.float32), np.zeros(1, np.uint8)
        n = 0
    else:
        n = len(masses)
    return int(emu.emu_min_rank(masses.ctypes.data_as(f32p), ranks.ctypes.data_as(u8p), n, np.float32(center), TOL_KINDS[tol[0]],
                                np.float32(tol[1]), np.float32(tol[2])))


def test_constants(emu):
    assert [emu.emu_depth_constants(k) for k in range(3)] == [11, LR.NO_PEAK, 10]


def _windows_spectrum(rng, sizes, tie_every=0):
    """sorted masses with sizes[w] peaks in 100-window w + 2, intensities random (every tie_every-th one repeated)"""
    masses, intens = [], []
    for w, size in enumerate(sizes):
        masses += sorted(rng.uniform((w + 2) * 100.0 + 0.01, (w + 3) * 100.0 - 0.01, size).astype(np.float32).tolist())
    intens = rng.lognormal(5.0, 1.0, len(masses)).astype(np.float32)
    if tie_every:
        for k in range(tie_every, len(intens), tie_every):
            intens[k] = intens[k - 1]
    return np.array(masses, np.float32), intens


def test_windows_of_1_10_11_and_40_peaks(emu):
    rng = np.random.default_rng(21)
    masses, intens = _windows_spectrum(rng, [1, 10, 11, 40])
    got, want = ranks_of(emu, masses, intens), LR.depth_ranks(masses, intens)
    assert np.array_equal(got, want)
    off = np.cumsum([0, 1, 10, 11, 40])
    assert list(got[:1]) == [1]
    assert sorted(got[off[1]:off[2]]) == list(range(1, 11))             # ten peaks: ranks 1..10, none capped
    assert sorted(got[off[2]:off[3]]) == list(range(1, 12))             # eleven: the last one is rank 11 as it stands
    assert sorted(got[off[3]:off[4]]) == list(range(1, 11)) + [11] * 30  # forty: thirty ranks stored as 11


def test_equal_intensities_inside_a_window(emu):
    rng = np.random.default_rng(22)
    masses, intens = _windows_spectrum(rng, [5, 14, 3], tie_every=2)
    got = ranks_of(emu, masses, intens)
    assert np.array_equal(got, LR.depth_ranks(masses, intens))
    # all equal: the ranks are the positions inside the window
    flat = np.full(len(masses), 7.0, np.float32)
    assert list(ranks_of(emu, masses, flat)) == list(range(1, 6)) + list(range(1, 12)) + [11, 11, 11] + [1, 2, 3]
    assert np.array_equal(ranks_of(emu, masses, flat), LR.depth_ranks(masses, flat))


def test_a_peak_at_exactly_300(emu):
    masses = np.array([299.99997, 300.0, 300.00003, 399.99997], np.float32)
    intens = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    assert [LR.window_of(m) for m in masses] == [2, 3, 3, 3]  # 300.0 opens window 3
    got = ranks_of(emu, masses, intens)
    assert list(got) == [1, 3, 2, 1] and np.array_equal(got, LR.depth_ranks(masses, intens))


def test_an_empty_spectrum_and_a_single_peak(emu):
    assert len(ranks_of(emu, [], [])) == 0
    assert min_rank_of(emu, [], [], 500.0, ("ppm", -10.0, 10.0)) == LR.NO_PEAK
    assert list(ranks_of(emu, [500.0], [3.0])) == [1]
    assert min_rank_of(emu, [500.0], [1], 500.0, ("ppm", -10.0, 10.0)) == 1
    assert min_rank_of(emu, [500.0], [1], 501.0, ("ppm", -10.0, 10.0)) == LR.NO_PEAK


def test_a_tolerance_window_that_spans_two_100_windows(emu):
    # 0.5 Da around 300.0: peaks of window 2 and of window 3, each ranked inside its own window
    masses = np.array([250.0, 299.7, 299.9, 300.1, 300.4, 350.0], np.float32)
    intens = np.array([9.0, 1.0, 2.0, 5.0, 6.0, 7.0], np.float32)
    ranks = ranks_of(emu, masses, intens)
    assert list(ranks) == [1, 3, 2, 3, 2, 1] and np.array_equal(ranks, LR.depth_ranks(masses, intens))
    tol = ("da", -0.5, 0.5)
    assert min_rank_of(emu, masses, ranks, 300.0, tol) == LR.min_rank(masses, ranks, 300.0, tol) == 2
    assert min_rank_of(emu, masses, ranks, 300.0, ("da", -0.15, 0.15)) == LR.min_rank(masses, ranks, 300.0, ("da", -0.15, 0.15)) == 2
    assert min_rank_of(emu, masses, ranks, 300.0, ("da", -0.05, 0.15)) == 3   # 300.1 alone
    assert min_rank_of(emu, masses, ranks, 300.0, ("da", -0.05, 0.05)) == LR.NO_PEAK


@pytest.mark.parametrize("tol", [("ppm", -10.0, 10.0), ("ppm", -500.0, 200.0), ("da", -0.3, 0.7), ("pct", -0.05, 0.05)])
def test_min_rank_equals_the_restatement_on_random_spectra(emu, tol):
    rng = np.random.default_rng(23)
    checked = hits = 0
    for n in (1, 2, 3, 37, 64, 65, 150, 700):
        masses = np.sort(rng.uniform(150.0, 1200.0, n).astype(np.float32))
        masses[n // 2:n // 2 + 2] = masses[n // 2]  # (two peaks of one mass)
        intens = np.round(rng.lognormal(3.0, 1.0, n)).astype(np.float32)  # (rounded: ties)
        ranks = ranks_of(emu, masses, intens)
        assert np.array_equal(ranks, LR.depth_ranks(masses, intens)), n
        centers = np.concatenate([masses, masses * np.float32(1.000009), rng.uniform(100.0, 1300.0, 40).astype(np.float32),
                                  [np.float32(0.0), np.float32(1e9), masses[0], masses[-1]]])
        for c in centers:
            got, want = min_rank_of(emu, masses, ranks, c, tol), LR.min_rank(masses, ranks, np.float32(c), tol)
            assert got == want, (n, float(c), got, want)
            # the same peaks as select_most_intense_peak looks at: a peak is found exactly when a rank is
            pk = emu.emu_most_intense(masses.ctypes.data_as(f32p), intens.ctypes.data_as(f32p), n, np.float32(c), TOL_KINDS[tol[0]],
                                      np.float32(tol[1]), np.float32(tol[2]))
            assert (pk >= 0) == (got != LR.NO_PEAK)
            checked += 1
            hits += got != LR.NO_PEAK
    assert checked > 2000 and hits > 800
