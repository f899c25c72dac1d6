"""sage_amd/csrc/crlog.h: cr_log1pf — the f32 `ln_1p` of OpenMSHyperScore, shared by the kernels and the host — compiled for the
host (tests/hostemu/ln1pf_emu.cpp) and held to libquadmath's 113-bit log1pq rounded ONCE to f32 on all 2^32 bit patterns.

The sweep asks libquadmath only where glibc's f64 log1p (< 1 ulp) lies within 8 f64 ulps of the midpoint of two floats (the
"hard" arguments: 45 positive ones) and takes the rounded f64 elsewhere; every 4099th pattern is audited with libquadmath
whatever the filter says.  Below |x| = 2^-40 the result must be the argument itself, bit for bit (a subnormal result's rounding
boundaries are not where the low bits of a double say).

It also takes a census of the PLATFORM's log1pf on the positive arguments from 2^-40 up — the reason this function exists: glibc
2.35 is one f32 ulp off the correctly rounded value on 0.65 % of them (9 149 215 of 1 409 286 144), so "the reference's value"
for a reference that calls the platform's log1pf is a property of the host's libm."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "ln1pf_emu.cpp")
LIB = os.path.join(HERE, "hostemu", "libln1pf_emu.so")
u32p, fp = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
THREADS = min(16, os.cpu_count() or 1)

# Rounding the correctly rounded f64 log1p to f32 is wrong for exactly these positive arguments (0x41078feb is 8.4726) ...
DOUBLE_ROUNDING = [0x35400003, 0x3710001B, 0x3EFD81AD, 0x41078FEB, 0x65D890D3, 0x6F31A8EC]
# ... and these negative ones
DOUBLE_ROUNDING_NEGATIVE = [0xB53FFFFD, 0xB70FFFE5, 0xBB0EC8C4]
# the positive arguments the filter sends to libquadmath (test_the_hard_arguments_are_the_listed_ones holds the list to the sweep)
HARD_POSITIVE = [
    0x35400003, 0x36DEDACE, 0x3710001B, 0x3770004B, 0x37C6E0E0, 0x3B9315C8, 0x3CF58230, 0x3DDBFEC3, 0x3EBE9143, 0x3EFD81AD,
    0x3F26C9AE, 0x41078FEB, 0x44BC2360, 0x464D572B, 0x4665A5A6, 0x46CA6A75, 0x4B773259, 0x4E599333, 0x4EE5F0E7, 0x50DA4BF6,
    0x542DFAC1, 0x55185F82, 0x5588E13B, 0x5B98E163, 0x5BF9890B, 0x5D800341, 0x5D8B2D5B, 0x5EE8984E, 0x5EFBCAAE, 0x5F64C24A,
    0x62B467BA, 0x63B134D9, 0x64E27FA3, 0x65D890D3, 0x66A8C860, 0x66ABBD63, 0x6914CB96, 0x6D1F23EB, 0x6E7054F2, 0x6F31A8EC,
    0x736CC271, 0x7405DEE8, 0x74896A73, 0x79E7EC37, 0x7D98B8F4]
HARD_NEGATIVE = [0xB3B504F3, 0xB53FFFFD, 0xB619776C, 0xB70FFFE5, 0xB76FFFB5, 0xB7C6E012, 0xBA800B50, 0xBB0EC8C4]


def load():
    csrc = os.path.join(HERE, "..", "sage_amd", "csrc")
    deps = [SRC, os.path.join(csrc, "crlog.h"), os.path.join(csrc, "crlog_tables.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        # (no -mfma, as in test_crlog.py: the header must not depend on the host having the instruction)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread", SRC,
                               "-o", LIB, "-lquadmath"])
    lib = C.CDLL(LIB)
    for f in (lib.emu_cr_log1pf, lib.emu_ref_ln1pf, lib.emu_libm_log1pf):
        f.argtypes = [fp, C.c_uint64, fp]
    lib.emu_sweep.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.c_uint32, u32p, u32p, u32p, u32p]
    return lib


def _apply(fn, bits):
    x = np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)
    out = np.empty_like(x)
    fn(x.ctypes.data_as(fp), len(x), out.ctypes.data_as(fp))
    return out.view(np.uint32)


def cr_log1pf(bits):
    """cr_log1pf on an array of f32 bit patterns -> bit patterns"""
    return _apply(load().emu_cr_log1pf, bits)


def ref_ln1pf(bits):
    """the reference: libquadmath's log1pq rounded once to f32, on bit patterns -> bit patterns"""
    return _apply(load().emu_ref_ln1pf, bits)


def libm_log1pf(bits):
    return _apply(load().emu_libm_log1pf, bits)


STATS = ("mismatches", "hard", "audited", "audit_failures", "libm_compared", "libm_wrong", "libm_max_ulp", "libm_max_ulp_arg")


def sweep(first, last, threads=THREADS, cap=256):
    """Patterns [first, last): (stats dict, mismatching patterns, hard arguments, arguments the platform's log1pf gets wrong) —
    of each list the first `cap` of the range, ascending."""
    st = (C.c_uint64 * 8)()
    lists = [np.zeros(cap, np.uint32) for _ in range(3)]
    n = np.zeros(3, np.uint32)
    load().emu_sweep(first, last, threads, st, cap, *[a.ctypes.data_as(u32p) for a in lists], n.ctypes.data_as(u32p))
    return (dict(zip(STATS, [int(v) for v in st])),) + tuple(a[:k].copy() for a, k in zip(lists, n))


_slices = {}


def slice_result(i):
    if i not in _slices:
        _slices[i] = sweep(i << 28, (i + 1) << 28)
    return _slices[i]


@pytest.mark.parametrize("i", range(16))
def test_every_bit_pattern(i):
    """Slice i of 16: patterns [i 2^28, (i + 1) 2^28)."""
    st, mism, hard, _ = slice_result(i)
    print(f"slice {i}: {st}")
    assert st["mismatches"] == 0, f"slice {i}: {st['mismatches']} patterns differ from the reference, first {[hex(v) for v in mism[:8]]}"
    assert st["audit_failures"] == 0, f"slice {i}: the filter disagrees with libquadmath on {st['audit_failures']} audited patterns"
    assert st["audited"] in (65488, 65489)  # every 4099th of 2^28


def test_the_hard_arguments_are_the_listed_ones():
    """What the filter sends to libquadmath over all 2^32 patterns is HARD_POSITIVE and HARD_NEGATIVE — the lists the aimed GPU
    worlds (tests/openms_worlds.py) take their hard arguments from."""
    hard = np.concatenate([slice_result(i)[2] for i in range(16)])
    assert [int(v) for v in hard] == HARD_POSITIVE + HARD_NEGATIVE
    assert set(DOUBLE_ROUNDING) <= set(HARD_POSITIVE) and set(DOUBLE_ROUNDING_NEGATIVE) <= set(HARD_NEGATIVE)


def test_the_platform_log1pf_is_not_correctly_rounded():
    """The census over the positive arguments from 2^-40 up to FLT_MAX.  Measured with glibc 2.35: 9 149 215 of 1 409 286 144
    (0.65 %) differ from the reference, on [1, 1e7] 2.4 %; the largest distance is 1 f32 ulp.  The
    floor of 0.5 % keeps the reason for cr_log1pf on record and fails if the sweep stops comparing."""
    st = [slice_result(i)[0] for i in range(8)]
    compared, wrong = sum(s["libm_compared"] for s in st), sum(s["libm_wrong"] for s in st)
    worst = max(st, key=lambda s: s["libm_max_ulp"])
    print(f"platform log1pf: {wrong} of {compared} positive arguments differ from the correctly rounded value "
          f"({100.0 * wrong / compared:.3f} %); largest distance {worst['libm_max_ulp']} f32 ulp at {worst['libm_max_ulp_arg']:#x}")
    assert compared == 0x7F800000 - 0x2B800000
    assert wrong >= 0.005 * compared
    assert worst["libm_max_ulp"] >= 1


def test_the_double_rounding_arguments_by_name():
    bits = np.array(DOUBLE_ROUNDING + DOUBLE_ROUNDING_NEGATIVE, dtype=np.uint32)
    ref = ref_ln1pf(bits)
    assert np.array_equal(cr_log1pf(bits), ref)
    assert [hex(v) for v in ref[:6]] == ["0x353fffff", "0x370ffff3", "0x3ecdeee1", "0x400fe5e7", "0x4254d1f9", "0x42845a89"]
    # what makes them special: the correctly rounded DOUBLE of ln(1 + x) is the midpoint of two floats, and rounding it again
    # goes to the even one — the wrong one.  (glibc's f64 log1p is correctly rounded on these nine.)
    d = np.log1p(bits.view(np.float32).astype(np.float64))
    assert np.all((d.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000))
    assert np.all(d.astype(np.float32).view(np.uint32) != ref)


def test_special_values():
    x = np.array([0.0, -0.0, -1.0, -1.0000001, -2.0, -np.inf, np.nan, np.inf, np.finfo(np.float32).max, 1e-45, -1e-45,
                  np.finfo(np.float32).tiny, 2.0 ** -29, np.nextafter(np.float32(2.0 ** -29), np.float32(0))], dtype=np.float32)
    y = cr_log1pf(x.view(np.uint32)).view(np.float32)
    assert y[0].view(np.uint32) == 0 and y[1].view(np.uint32) == 0x80000000          # +0 -> +0, -0 -> -0
    assert y[2] == -np.inf and np.isnan(y[3:7]).all() and y[7] == np.inf
    ref = ref_ln1pf(x.view(np.uint32)).view(np.float32)
    assert np.array_equal(y[8:].view(np.uint32), ref[8:].view(np.uint32))
    assert np.array_equal(y[9:12].view(np.uint32), x[9:12].view(np.uint32))             # subnormals and FLT_MIN: the argument


def test_the_second_readings_ln_1p_is_a_third_route():
    """tests/second_reading.py: ln_1p_f32 (mpmath at 200 bits, the nearest f32 by exact comparison) equals the reference on the
    hard arguments, on arguments the platform's log1pf gets wrong and on random ones."""
    import second_reading as SR
    rng = np.random.default_rng(3)
    wrong = sweep(0x41000000, 0x41000000 + 20000, threads=1, cap=100)[3]
    assert len(wrong) == 100
    bits = np.concatenate([np.array(HARD_POSITIVE + HARD_NEGATIVE, dtype=np.uint32), wrong,
                           rng.integers(0x2B800000, 0x7F800000, 200).astype(np.uint32),
                           rng.integers(0xAB800000, 0xBF800000, 100).astype(np.uint32),
                           np.array([0, 0x80000000, 0xBF800000, 0xC0000000, 0x7F800000, 0x7FC00000, 1, 0x80000001], dtype=np.uint32)])
    ref = ref_ln1pf(bits).view(np.float32)
    mine = np.array([SR.ln_1p_f32(v) for v in bits.view(np.float32)], dtype=np.float32)
    assert np.array_equal(np.isnan(mine), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(mine[ok].view(np.uint32), ref[ok].view(np.uint32))
