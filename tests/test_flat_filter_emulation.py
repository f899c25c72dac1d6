"""CPU tests of the flat bitmap filter's bookkeeping (sage_amd/csrc/core.h: flat_octets, flat_item_k, flat_item_base /
flat_item_ion, flat_stride, flat_area_bytes, flat_mask_word), compiled for the host (tests/hostemu/flat_filter_emu.cpp) and replayed lane by lane the way
kernels.hip: score_candidates runs a 64-ion chunk: every item of the flattened list belongs to exactly one (owner, octet), and the
masks assembled from the workers' bytes are the per-lane filter's, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "flat_filter_emu.cpp")
LIB = os.path.join(HERE, "hostemu", "libflat_filter_emu.so")
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
f32p = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "..", "sage_amd", "csrc", "core.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    for name in ("emu_flat_octets", "emu_flat_area_bytes", "emu_flat_route_wins", "emu_pbm_words", "emu_flat_items", "emu_flat_masks"):
        getattr(lib, name).restype = C.c_uint32
    lib.emu_flat_octets.argtypes = [C.c_uint32]
    lib.emu_flat_area_bytes.argtypes = [C.c_uint32, C.c_uint32]
    lib.emu_flat_route_wins.argtypes = [C.c_uint32, C.c_uint32]
    lib.emu_flat_items.argtypes = [u32p, u32p, u32p]
    lib.emu_flat_masks.argtypes = [f32p, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u64p, u64p]
    return lib


def item_lists():
    rng = np.random.default_rng(5)
    lists = {"all zero": np.zeros(64, np.uint32), "all 8": np.full(64, 8, np.uint32)}
    for lane in (0, 17, 63):
        one = np.zeros(64, np.uint32)
        one[lane] = 1 + lane % 8
        lists[f"lane {lane} only"] = one
    t64 = np.ones(64, np.uint32)
    lists["a total of exactly 64"] = t64
    t65 = t64.copy()
    t65[40] = 2
    lists["a total of exactly 65"] = t65
    inter = np.zeros(64, np.uint32)
    inter[1::2] = rng.integers(1, 9, 32)
    lists["zeros interleaved"] = inter
    inter2 = np.zeros(64, np.uint32)
    inter2[::3] = 8
    lists["zeros between full lanes"] = inter2
    for i in range(200):
        c = rng.integers(0, 9, 64).astype(np.uint32)
        c[rng.random(64) < rng.random()] = 0
        lists[f"random {i}"] = c
    return lists


def test_every_item_has_one_owner_and_octet(emu):
    for name, counts in item_lists().items():
        total = int(counts.sum())
        owner = np.full(max(total, 1), 0xFFFFFFFF, np.uint32)
        k = np.full(max(total, 1), 0xFFFFFFFF, np.uint32)
        n = emu.emu_flat_items(counts.ctypes.data_as(u32p), owner.ctypes.data_as(u32p), k.ctypes.data_as(u32p))
        assert n == total, name
        pairs = list(zip(owner[:total].tolist(), k[:total].tolist()))
        assert all(kk < counts[o] for o, kk in pairs), name
        # every (owner, octet) is hit exactly once, and in the order of the flattened list
        assert pairs == [(lane, j) for lane in range(64) for j in range(int(counts[lane]))], name


def test_octets_area_and_choice(emu):
    for n in range(0, 65):
        assert emu.emu_flat_octets(n) == (n + 7) // 8
    for total in range(0, 513):
        for nch in (1, 2, 3):
            # every stripe word-aligned, and the last owner's three-word read inside the area
            need = emu.emu_flat_area_bytes(total, nch)
            stride = (need - 12) // nch
            assert stride % 4 == 0 and stride >= total
            if total:
                assert (nch - 1) * stride + ((total - 1) & ~3) + 12 <= need
    assert not emu.emu_flat_route_wins(0, 8)
    assert emu.emu_flat_route_wins(64, 8) and not emu.emu_flat_route_wins(512, 8) and not emu.emu_flat_route_wins(8, 1)


@pytest.mark.parametrize("nfz_max", [1, 2, 3, 5])
def test_masks_from_bytes_equal_the_per_lane_masks(emu, nfz_max):
    rng = np.random.default_rng(100 + nfz_max)
    words = emu.emu_pbm_words()
    special = [1, 2, 7, 8, 9, 63, 64, 65]
    stride = 136  # two chunks of ions and the table's padding of 8
    for trial in range(60):
        nions = rng.integers(0, 129 if trial % 2 else 65, 64).astype(np.uint32)  # (odd trials: candidates of up to two chunks)
        nions[rng.permutation(64)[:len(special)]] = special
        if trial % 3 == 0:
            nions[rng.random(64) < 0.5] = 0  # lanes without a candidate
        if trial == 1:
            nions[:] = 64
        if trial == 2:
            nions[:] = 0
            nions[31] = 1
        if trial == 3:
            nions[:] = 65  # every lane: a full chunk and a second one of one ion
        nfz = rng.integers(1, nfz_max + 1, 64).astype(np.uint32)
        if trial % 5 == 4:
            nfz[:] = nfz_max
        bitmap = rng.integers(0, 2**32, words, dtype=np.uint64).astype(np.uint32)
        if trial % 4 == 0:
            bitmap &= rng.integers(0, 2**32, words, dtype=np.uint64).astype(np.uint32)  # sparser
        if trial == 7:
            bitmap[:] = 0xFFFFFFFF
        ions = rng.uniform(50.0, 6000.0, 64 * stride).astype(np.float32)
        for j0 in range(0, max(int(nions.max()), 1), 64):  # the kernel's chunk loop
            n_here = np.clip(nions.astype(np.int64) - j0, 0, 64)
            m_flat = np.zeros(192, np.uint64)
            m_lane = np.zeros(192, np.uint64)
            trips = emu.emu_flat_masks(ions.ctypes.data_as(f32p), stride, j0, nions.ctypes.data_as(u32p), nfz.ctypes.data_as(u32p),
                                       bitmap.ctypes.data_as(u32p), m_flat.ctypes.data_as(u64p), m_lane.ctypes.data_as(u64p))
            octets = int((((n_here + 7) // 8) * ((nfz <= 3) & (n_here > 0))).sum())
            assert trips == (octets + 63) // 64
            assert np.array_equal(m_flat, m_lane), (nfz_max, trial, j0)
            # a lane's masks reach no further than its ions of this chunk
            assert not (m_lane.reshape(3, 64) >> n_here.astype(np.uint64).clip(max=63)[None, :] >> (n_here == 64)[None, :].astype(np.uint64)).any()
            if nfz_max <= 3 and n_here.any():
                assert m_lane[:64].any() or trial == 2 or j0
