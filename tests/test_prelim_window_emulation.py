"""CPU test of scalar_query_window (sage_amd/csrc/core.h), compiled for the host (tests/hostemu/prelim_window_emu.cpp): the one-thread
form of IndexedDatabase::query whose result a resident batch's upload leaves in the schedule records, against an independent numpy
statement — searchsorted on the total-order keys, then the edge rule of database.rs:526-531."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "prelim_window_emu.cpp")
LIB = os.path.join(HERE, "hostemu", "libprelim_window_emu.so")
u32p = C.POINTER(C.c_uint32)
f32p = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "..", "sage_amd", "csrc", "core.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.emu_scalar_query_window.argtypes = [f32p, C.c_uint32, C.c_float, C.c_float, u32p]
    lib.emu_scalar_query_window.restype = None
    lib.emu_order_key.argtypes = [C.c_float]
    lib.emu_order_key.restype = C.c_int32
    return lib


def total_order_keys(x):
    """f32::total_cmp as integers, stated on the bit patterns: negative floats order by descending magnitude bits"""
    bits = np.asarray(x, np.float32).view(np.uint32).astype(np.int64)
    neg = bits >= 2**31
    return np.where(neg, -(bits - 2**31) - 1, bits)


def numpy_window(masses, plo, phi):
    """IndexedDatabase::query's slots [left, right] and the peptide range [first, end) after the edge rule, from searchsorted"""
    keys = total_order_keys(masses)
    klo, khi = int(total_order_keys([plo])[0]), int(total_order_keys([phi])[0])
    a = int(np.searchsorted(keys, klo, side="left"))  # partition_point(key < klo)
    left = a - 1 if a else 0
    right = left + int(np.searchsorted(keys[left:], khi, side="right"))  # partition_point(key <= khi), from `left` on
    first, end = left, right
    with np.errstate(invalid="ignore"):
        if left < len(masses) and not (masses[left] >= np.float32(plo)):
            first = left + 1
        if right < len(masses) and masses[right] <= np.float32(phi):
            end = right + 1
    return [left, right, first, end]


def mass_arrays():
    rng = np.random.default_rng(3)
    f = np.float32
    arrays = {
        "np = 0": np.zeros(0, f),
        "np = 1": np.array([1000.5], f),
        "np = 1, zero": np.array([0.0], f),
        "duplicates": np.sort(np.repeat(rng.uniform(500, 5000, 40).astype(f), rng.integers(1, 5, 40))),
        "all equal": np.full(17, 1234.5, f),
        "signed zeros": np.array([-3.0, -0.0, -0.0, 0.0, 0.0, 2.0, 2.0, 7.5], f),
        "negative masses": np.sort(rng.uniform(-2000, 2000, 300).astype(f)),
        "dense": np.sort(rng.uniform(799.0, 801.0, 1000).astype(f)),
    }
    for name, a in arrays.items():
        keys = total_order_keys(a)
        assert np.all(keys[1:] >= keys[:-1]), name  # ascending in the total order (-0.0 before +0.0)
    return arrays


def windows_for(a):
    rng = np.random.default_rng(len(a) + 11)
    f = np.float32
    nan = f("nan")
    lo_edge = f(a[0]) if len(a) else f(0)
    hi_edge = f(a[-1]) if len(a) else f(0)
    w = [(lo_edge - f(10), lo_edge - f(5)), (hi_edge + f(5), hi_edge + f(10)),  # below the first, above the last
         (lo_edge - f(10), hi_edge + f(10)), (f(-0.0), f(0.0)), (f(0.0), f(-0.0)),
         (nan, nan), (nan, f(1000)), (f(1000), nan), (-nan, nan), (f("-inf"), f("inf")), (f("inf"), f("-inf"))]
    for m in list(a[:: max(1, len(a) // 12)]) + [lo_edge, hi_edge]:
        m = f(m)
        up, down = np.nextafter(m, f("inf")), np.nextafter(m, f("-inf"))
        w += [(m, m), (m, up), (down, m), (up, up), (down, down), (m, m + f(0.01)), (m - f(0.01), m),  # bounds equal to a stored mass
              (up, down), (m + f(3), m - f(3))]  # inverted
    for _ in range(150):
        c = f(rng.uniform(lo_edge - 50, hi_edge + 50))
        d = f(abs(rng.normal(0, 0.5)))
        w.append((c - d, c + d))
        if rng.random() < 0.2:
            w.append((c + d, c - d))
        if rng.random() < 0.2:
            w.append((c, c))  # empty unless c is stored
    return w


def test_scalar_window_against_numpy(emu):
    out = np.zeros(4, np.uint32)
    checked = nonempty = empty = inverted = edge_first = edge_end = 0
    for name, a in mass_arrays().items():
        buf = np.ascontiguousarray(a) if len(a) else np.zeros(1, np.float32)
        for plo, phi in windows_for(a):
            emu.emu_scalar_query_window(buf.ctypes.data_as(f32p), len(a), float(plo), float(phi), out.ctypes.data_as(u32p))
            want = numpy_window(a, plo, phi)
            assert out.tolist() == want, (name, float(plo), float(phi), out.tolist(), want)
            checked += 1
            nonempty += want[3] > want[2]
            empty += want[3] <= want[2]
            inverted += bool(plo > phi)
            edge_first += want[2] != want[0]
            edge_end += want[3] != want[1]
    assert checked > 1000 and nonempty > 100 and empty > 100 and inverted > 50 and edge_first > 100 and edge_end > 0
    # (end == right + 1 needs a mass beyond phi in the total order that is <= phi as a number: +0.0 against -0.0, or right == left)


def test_order_key_is_the_total_order(emu):
    vals = np.array([float("-inf"), -5.0, -0.0, 0.0, 1e-45, 5.0, float("inf")], np.float32)
    assert [emu.emu_order_key(float(v)) for v in vals] == total_order_keys(vals).tolist()
    assert emu.emu_order_key(float("nan")) > emu.emu_order_key(float("inf"))  # (a positive NaN sorts behind everything)


def test_scalar_window_against_the_oracles_query(emu):
    """left / right against IndexedDatabase::query of the oracle (oracle_lib.OracleDb.page_search returns its pre_idx_lo / pre_idx_hi)
    over a small database's peptide masses: ppm, Da and one-sided tolerances, centres at, beside and between stored masses, beyond both
    ends — bounds that equal a stored mass exactly among them."""
    import oracle_lib
    from sage_amd.api import DatabaseParameters, Tolerance
    from sage_amd.synthetic import synthetic_fasta

    orc = oracle_lib.OracleDb.build(synthetic_fasta(40, seed=13), DatabaseParameters(bucket_size=1024, enzyme=dict(
        missed_cleavages=1, cleave_at="KR", restrict="P"), static_mods={"C": 57.0215}, variable_mods={"M": [15.9949]}))
    mono = np.ascontiguousarray(orc.arrays()["pep_mono"])
    assert len(mono) > 1000 and np.all(np.diff(mono) >= 0) and np.any(np.diff(mono) == 0)  # ascending, with equal masses
    f = np.float32
    rng = np.random.default_rng(17)
    stored = mono[rng.integers(0, len(mono), 60)]
    centres = np.concatenate([stored, np.nextafter(stored[:20], f("inf")), np.nextafter(stored[:20], f("-inf")),
                              stored[:20] + f(1.0), stored[:20] - f(0.5),
                              rng.uniform(mono[0] - 5, mono[-1] + 5, 200).astype(f),
                              [mono[0], mono[-1], mono[0] - f(50), mono[-1] + f(50), f(0.0)]]).astype(f)
    tols = [Tolerance("ppm", -10.0, 10.0), Tolerance("ppm", -50.0, 20.0), Tolerance("da", -1.0, 1.0), Tolerance("da", -0.5, 0.0),
            Tolerance("da", 0.0, 0.5), Tolerance("da", 0.0, 0.0), Tolerance("da", -1.0, 0.0), Tolerance("da", -3.0, 3.0),
            Tolerance("da", 0.25, -0.25), Tolerance("pct", -0.01, 0.01)]
    ftol = Tolerance("ppm", -10.0, 10.0)
    out = np.zeros(4, np.uint32)
    in_mono = set(mono.tolist())
    checked = on_a_mass = several = 0
    for tol in tols:
        for c in centres:
            plo, phi = oracle_lib.tol_bounds(tol, float(c))  # Tolerance::bounds in f32, as window_max_kernel computes them (tol_bounds)
            _, lo, hi = orc.page_search(float(c), tol, ftol, 500.0, cap=1)
            emu.emu_scalar_query_window(mono.ctypes.data_as(f32p), len(mono), plo, phi, out.ctypes.data_as(u32p))
            assert (int(out[0]), int(out[1])) == (lo, hi), (tol, float(c), plo, phi, out.tolist(), lo, hi)
            assert out.tolist() == numpy_window(mono, f(plo), f(phi))
            checked += 1
            on_a_mass += plo in in_mono or phi in in_mono
            several += hi - lo > 2
    assert checked == len(tols) * len(centres) and on_a_mass > 100 and several > 500
