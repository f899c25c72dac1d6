"""Precursor purity without a device: sage_amd/csrc/purity.h compiled for the host (tests/hostemu/purity_emu.cpp)
against the plain restatement (tests/purity_reference.py), bit for bit, on the named worlds (tests/purity_worlds.py) and on random
ones; answers computed by hand; assign_ms1; the checks sage_hip_precursor_purity makes before it touches a device; the exported
symbols; the row builder against the native writer.  (The kernel itself needs a device: tests/test_gpu_purity.py.)"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import purity_reference as REF
import purity_worlds as W
from sage_amd import _lib as L
from sage_amd import api, cli, output

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "purity_emu.cpp")
LIB = os.path.join(HERE, "hostemu", "libpurity_emu.so")
CSRC = os.path.join(HERE, "..", "sage_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("purity.h", "core.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
F = np.float32
fp, dp, up, u8p, u64p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_uint32, C.c_uint8, C.c_uint64))


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        subprocess.check_call(["g++", "-O2", *FLAGS, "-fPIC", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.emu_purity.argtypes = [C.c_uint64, u64p, fp, fp, C.c_uint64, u64p, fp, u8p, fp, fp, C.c_float, C.c_float, C.c_float, C.c_uint32,
                               up, up, dp, dp, dp, fp]
    lib.emu_purity.restype = C.c_int
    return lib


def flatten(batches):
    """the spectra of every batch as one (peak_off, mz, intensity)"""
    off, mz, it, last = [np.zeros(1, np.uint64)], [np.zeros(0, F)], [np.zeros(0, F)], np.uint64(0)
    for b in batches:
        off.append(b.peak_off[1:] + last)
        last = last + b.peak_off[-1]
        mz.append(b.mz)
        it.append(b.intensities)
    return np.ascontiguousarray(np.concatenate(off)), np.ascontiguousarray(np.concatenate(mz)), np.ascontiguousarray(np.concatenate(it))


def run_emu(emu, w):
    off, mz, it = flatten(w.batches)
    n = len(w.ms1_index)
    out = {"n_window": np.zeros(n, np.uint32), "n_matched": np.zeros(n, np.uint32), "total": np.zeros(n), "matched": np.zeros(n),
           "below": np.zeros(n), "purity": np.zeros(n, F)}
    idx, pmz, z = (np.ascontiguousarray(a) for a in (w.ms1_index, w.mz, w.charge))
    lo = None if w.lo is None else np.ascontiguousarray(w.lo)
    hi = None if w.hi is None else np.ascontiguousarray(w.hi)
    rc = emu.emu_purity(len(off) - 1, L.as_ptr(off, C.c_uint64), L.as_ptr(mz, C.c_float), L.as_ptr(it, C.c_float), n,
                        L.as_ptr(idx, C.c_uint64), L.as_ptr(pmz, C.c_float), L.as_ptr(z, C.c_uint8),
                        None if lo is None else L.as_ptr(lo, C.c_float), None if hi is None else L.as_ptr(hi, C.c_float), w.ppm,
                        w.default[0], w.default[1], w.max_isotope, L.as_ptr(out["n_window"], C.c_uint32),
                        L.as_ptr(out["n_matched"], C.c_uint32), L.as_ptr(out["total"], C.c_double), L.as_ptr(out["matched"], C.c_double),
                        L.as_ptr(out["below"], C.c_double), L.as_ptr(out["purity"], C.c_float))
    assert rc == 0
    return out


@pytest.mark.parametrize("name", W.NAMES)
def test_emulation_equals_the_restatement(emu, name):
    W.assert_equal(run_emu(emu, W.world(name)), W.reference(name), name)


def test_emulation_equals_the_restatement_on_random_worlds(emu):
    rng = np.random.default_rng(2024)
    for trial in range(40):
        spectra = []
        for _ in range(int(rng.integers(1, 6))):
            n = int(rng.integers(0, 300))
            m = rng.uniform(400.0, 404.0, n).astype(F)
            if rng.random() < 0.5:
                m = np.sort(m)
            if n and rng.random() < 0.2:
                m[rng.integers(n)] = np.nan
            it = rng.lognormal(6.0, 2.0, n).astype(F)
            if n and rng.random() < 0.3:
                it[rng.integers(n)] = rng.choice([np.nan, np.inf, -np.inf, -1.0, -0.0])
            spectra.append((m, it))
        nq = int(rng.integers(0, 40))
        idx = rng.integers(0, len(spectra), nq).astype(np.uint64)
        idx[rng.random(nq) < 0.1] = REF.NO_MS1
        lo = np.where(rng.random(nq) < 0.3, np.nan, -rng.uniform(0.0, 1.5, nq)).astype(F)
        hi = np.where(rng.random(nq) < 0.1, np.nan, rng.uniform(0.0, 1.5, nq)).astype(F)
        w = W.World([W.batch(spectra)], idx, rng.uniform(399.5, 404.5, nq).astype(F), rng.integers(0, 7, nq).astype(np.uint8),
                    None if trial % 5 == 0 else lo, None if trial % 5 == 0 else hi, ppm=float(rng.choice([0.0, 5.0, 10.0, 50.0, 500.0])),
                    max_isotope=int(rng.choice([0, 1, 4, 16])), default=(-float(rng.uniform(0.1, 1.0)), float(rng.uniform(0.1, 1.0))))
        want = REF.run(w.batches, w.ms1_index, w.mz, w.charge, w.lo, w.hi, w.ppm, w.max_isotope, w.default)
        W.assert_equal(run_emu(emu, w), want, f"random {trial}")


def test_the_worlds_sit_on_their_seams():
    """what the named worlds claim to hold, asserted on the restatement's own answers"""
    w, want = W.world("populations_k4"), W.reference("populations_k4")
    assert want["n_window"].tolist() == w.notes["populations"] == [0, 1, 2, 63, 64, 65, 129, 1000]
    assert want["purity"][0] == F(-1.0) and (want["n_matched"][1:] >= 1).all()
    assert W.reference("populations_unsorted")["n_window"].tolist() == w.notes["populations"]
    want = W.reference("order_case")
    assert want["total"].tolist() == W.world("order_case").notes["totals"] == [2.0 ** 53, 2.0 ** 53 + 2.0, 2.0 ** 53, 2.0 ** 53 + 2.0]
    # a peak on each bound is inside, its neighbours one ulp outside are not: the counts differ between k = 0, 4, 16 and from a run
    # whose peaks were all moved one ulp outwards
    e0, e4, e16 = (W.reference(f"edges_k{k}") for k in (0, 4, 16))
    assert (e0["n_matched"] <= e4["n_matched"]).all() and (e4["n_matched"] <= e16["n_matched"]).all()
    assert e0["n_matched"].sum() < e4["n_matched"].sum()
    # a peak meeting two k is counted once: at 400 ppm and charge 6 the bounds of k = 0 and k = 1 overlap, peaks of the window lie in
    # both, and the count of matched peaks is the count of peaks, not of (peak, k) pairs
    w2, two = W.world("two_k"), W.reference("two_k")
    b = W.bounds_of(w2.mz[6], 6, w2.lo[6], w2.hi[6], 400.0, 4)
    peaks = w2.batches[0].mz
    in_both = (peaks >= b[0]) & (peaks <= b[1]) & (peaks >= b[2]) & (peaks <= b[3]) & (peaks >= b[4]) & (peaks <= b[5])
    per_k = sum(int(((peaks >= b[0]) & (peaks <= b[1]) & (peaks >= b[2 + 2 * k]) & (peaks <= b[3 + 2 * k])).sum()) for k in range(5))
    assert w2.charge[6] == 6 and in_both.sum() >= 7 and two["n_matched"][6] < per_k and (two["n_matched"] <= two["n_window"]).all()
    sizes = W.reference("sizes_k4")
    world = W.world("sizes_k4")
    none = world.ms1_index == REF.NO_MS1
    assert none.sum() == 5 and (sizes["purity"][none] == F(-1.0)).all() and not sizes["total"][none].any()
    assert sizes["n_window"].max() >= 900 and (sizes["n_matched"] > 1).sum() > 50 and (sizes["below"] > 0).sum() > 20
    odd = W.reference("odd_intensities")
    assert np.isnan(odd["total"][0]) and odd["total"][1] == np.inf and odd["total"][2] == -np.inf and np.isnan(odd["total"][7])
    assert odd["total"][6] == 0.0 and not np.signbit(odd["total"][6]) and np.isnan(odd["purity"][6]) and odd["n_window"][6] == 30


def test_hand_computed_answers(emu):
    # a window of three peaks, 300 / 100 / 0, the first on the precursor: purity 300 / 400
    sp = (np.array([499.0, 500.0, 500.2, 500.4, 502.0], F), np.array([7.0, 300.0, 100.0, 0.0, 9.0], F))
    w = W.World([W.batch([sp])], np.zeros(1, np.uint64), np.array([500.0], F), np.array([2], np.uint8))
    for got in (REF.run(w.batches, w.ms1_index, w.mz, w.charge), run_emu(emu, w)):
        assert got["n_window"][0] == 3 and got["n_matched"][0] == 1 and got["total"][0] == 400.0 and got["matched"][0] == 300.0
        assert got["purity"][0] == F(0.75) and got["below"][0] == 0.0
    # charge 2, isotopes at +0.501675 and +1.00335 inside a window of (-0.7, 1.2); a peak one neutron below at -0.501675 counts as
    # `below` and — inside the window — as interference
    mz0 = 600.0
    m = np.array([mz0 - 0.501675, mz0, mz0 + 0.25, mz0 + 0.501675, mz0 + 1.00335, mz0 + 1.5], F)
    it = np.array([50.0, 1000.0, 200.0, 500.0, 250.0, 4000.0], F)
    w = W.World([W.batch([(m, it)])], np.zeros(1, np.uint64), np.array([mz0], F), np.array([2], np.uint8), np.array([-0.7], F), np.array([1.2], F))
    for got in (REF.run(w.batches, w.ms1_index, w.mz, w.charge, w.lo, w.hi), run_emu(emu, w)):
        assert got["n_window"][0] == 5 and got["n_matched"][0] == 3 and got["total"][0] == 2000.0 and got["matched"][0] == 1750.0
        assert got["below"][0] == 50.0 and got["purity"][0] == F(0.875)
    # unknown charge: only the precursor's own peak is matched, nothing is `below`
    w.charge = np.array([0], np.uint8)
    for got in (REF.run(w.batches, w.ms1_index, w.mz, w.charge, w.lo, w.hi), run_emu(emu, w)):
        assert got["n_matched"][0] == 1 and got["matched"][0] == 1000.0 and got["below"][0] == 0.0 and got["purity"][0] == F(0.5)
    # no peak in the window: -1, every sum +0.0 — `below` too
    w = W.World([W.batch([(m, it)])], np.zeros(1, np.uint64), np.array([mz0 + 0.76], F), np.array([2], np.uint8), np.array([-0.1], F), np.array([0.1], F),
                ppm=200.0)
    for got in (REF.run(w.batches, w.ms1_index, w.mz, w.charge, w.lo, w.hi, ppm=200.0), run_emu(emu, w)):
        assert got["n_window"][0] == 0 and got["purity"][0] == F(-1.0) and got["below"][0] == 0.0 and got["total"][0] == 0.0


def _with_files(n, file_ids, times):
    b = W.batch([(np.zeros(0, F), np.zeros(0, F))] * n, times=np.array(times, F))
    b.file_id = np.array(file_ids, np.uint32)
    return b


def test_assign_ms1():
    none = REF.NO_MS1
    # two files interleaved over two batches; equal times in file 0 (spectra 1 and 3); file 2 has no MS1 at all
    batches = [_with_files(4, [0, 0, 1, 0], [1.0, 2.0, 1.5, 2.0]), _with_files(3, [1, 0, 1], [2.5, 3.0, 0.5])]
    fid = [0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 0]
    t = [0.5, 1.0, 1.99, 2.0, 9.0, 0.4, 0.5, 1.5, 2.6, 1.0, np.nan]
    want = [none, 0, 0, 3, 5, none, 6, 2, 4, none, none]
    assert REF.assign_ms1(batches, fid, t).tolist() == want
    assert api.assign_ms1(batches, fid, t).tolist() == want
    assert api.assign_ms1([], fid, t).tolist() == [none] * len(fid) and api.NO_MS1 == none
    assert api.assign_ms1(batches, [], []).tolist() == []
    rng = np.random.default_rng(5)
    for _ in range(20):
        batches = [_with_files(k, rng.integers(0, 3, k), rng.integers(0, 8, k).astype(F)) for k in rng.integers(0, 12, 3)]
        fid, t = rng.integers(0, 4, 50), rng.integers(-1, 9, 50).astype(F) + F(0.5) * rng.integers(0, 2, 50)
        assert api.assign_ms1(batches, fid, t).tolist() == REF.assign_ms1(batches, fid, t).tolist()


def purity_call(w, n_queries=None, **settings):
    """sage_hip_precursor_purity on a World through ctypes -> the status"""
    n = len(w.ms1_index) if n_queries is None else n_queries
    r = api.PurityResult(np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, F), 0, 0, {})
    cb = [b.to_c() for b in w.batches]
    arr = (L.SageRawBatch * max(len(cb), 1))(*cb)
    st = dict(ppm_tolerance=10.0, default_isolation_lo=-0.5, default_isolation_hi=0.5, max_isotope=4)
    st.update(settings)
    idx, mz, z = (np.ascontiguousarray(a) for a in (w.ms1_index, w.mz, w.charge))
    cin = L.SagePurityInput(len(cb), arr, n, L.as_ptr(idx, C.c_uint64), L.as_ptr(mz, C.c_float), L.as_ptr(z, C.c_uint8), None, None,
                            L.SagePuritySettings(**st))
    keep = []
    cout = r.to_c(keep)
    return L.load().sage_hip_precursor_purity(0, C.byref(cin), C.byref(cout)), r, cin, cout


def test_validation_comes_before_the_device():
    lib = L.load()
    err = lambda: lib.sage_hip_last_error().decode()
    w = W.world("nan_mz")
    assert purity_call(w, max_isotope=17)[0] == 1 and "max_isotope" in err()
    for bad in (-1.0, float("nan"), float("inf")):
        assert purity_call(w, ppm_tolerance=bad)[0] == 1 and "ppm_tolerance" in err()
    out_of_range = W.World(w.batches, np.array([3], np.uint64), w.mz[:1], w.charge[:1])
    assert purity_call(out_of_range)[0] == 1 and "ms1_index" in err()
    assert purity_call(W.World(w.batches, np.array([2 ** 64 - 2], np.uint64), w.mz[:1], w.charge[:1]))[0] == 1
    rc, r, cin, cout = purity_call(w)
    for name in ("ms1_index", "precursor_mz", "charge"):
        broken = L.SagePurityInput.from_buffer_copy(cin)
        setattr(broken, name, None)
        assert lib.sage_hip_precursor_purity(0, C.byref(broken), C.byref(cout)) == 1 and "null array" in err(), name
    for name in ("n_window", "n_matched", "total", "matched", "below", "purity"):
        broken = L.SagePurityOutput.from_buffer_copy(cout)
        setattr(broken, name, None)
        assert lib.sage_hip_precursor_purity(0, C.byref(cin), C.byref(broken)) == 1 and "null array" in err(), name
    assert lib.sage_hip_precursor_purity(0, None, C.byref(cout)) == 1 and lib.sage_hip_precursor_purity(0, C.byref(cin), None) == 1
    # empty calls: fine without a device, nothing launched
    rc, r, _, cout = purity_call(w, n_queries=0)
    assert rc == 0 and cout.n_sorted_spectra == 0 and cout.n_scanned_spectra == 0 and cout.device_ms == 0.0
    none = W.world("no_ms1_only")
    rc, r, _, cout = purity_call(none)
    assert rc == 0 and (r.purity == F(-1.0)).all() and not r.total.any() and not r.n_window.any() and cout.device_ms == 0.0
    some_none = W.World(w.batches, np.full(2, REF.NO_MS1, np.uint64), w.mz[:2], w.charge[:2])
    rc, r, _, cout = purity_call(some_none)
    assert rc == 0 and (r.purity == F(-1.0)).all() and cout.kernel_ms == 0.0


def test_abi_version_and_exported_symbols():
    lib = L.load()
    assert lib.sage_hip_abi_version() == 6
    new = ["sage_hip_precursor_purity", "sage_hip_write_purity"]
    assert all(s in L.EXPORTED_SYMBOLS for s in new)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(HERE, "..", "include", "sage_hip.h")).read()
    for s in new:
        assert f" T {s}\n" in dynamic, f"{s} is not exported"
        assert f" {s}(" in header, f"{s} is not declared in sage_hip.h"
    assert C.sizeof(L.SagePuritySettings) == 16 and C.sizeof(L.SagePurityInput) == 8 + 8 + 8 + 5 * 8 + 16
    assert C.sizeof(L.SagePurityOutput) == 6 * 8 + 2 * 8 + 3 * 4 + 4


def test_settings_keys():
    assert cli.purity_settings({}) == (False, {"ppm_tolerance": 10.0, "max_isotope": 4, "default_isolation": (-0.5, 0.5)})
    on, st = cli.purity_settings({"precursor_purity": True, "purity_settings": {"ppm_tolerance": 5, "max_isotope": 2, "default_isolation": [-1, 2]}})
    assert on and st == {"ppm_tolerance": 5.0, "max_isotope": 2, "default_isolation": (-1.0, 2.0)}
    for bad in ({"max_isotope": 17}, {"max_isotope": -1}, {"ppm_tolerance": -1}, {"ppm_tolerance": float("nan")}):
        with pytest.raises(SystemExit):
            cli.purity_settings({"purity_settings": bad})


def test_purity_rows_and_native_writer(tmp_path):
    n = 5
    r = api.PurityResult(np.array([3, 0, 1000, 1, 2], np.uint32), np.array([1, 0, 7, 1, 0], np.uint32),
                         np.array([400.0, 0.0, 1.5e300, np.nan, 2.0 ** 53 + 2.0]), np.array([300.0, 0.0, 1e-300, np.inf, -0.0]),
                         np.array([0.0, 0.0, 0.1, -np.inf, 5e-324]), np.array([0.75, -1.0, 0.0, np.nan, 1e-45], F), 0, 0, {})
    files = ["a.mzML", "tab\tname.mzML"]
    args = ([11, 12, 13, 2 ** 40, 15], files, [0, 1, 1, 0, 1], ["scan=7", "controllerType=0 scan=9", 'q"uote', "x", "y"],
            [2, 0, 255, 3, 1], ["scan=1", "", "scan=5", None, "scan=6"], np.array([-0.5, -0.7, np.nan, -1e-3, -2.0], F),
            np.array([0.5, 0.9, 0.25, 1e3, np.inf], F), r)
    rows = output.purity_rows(*args)
    assert rows[0] == ["11", "a.mzML", "scan=7", "2", "scan=1", "-0.5", "0.5", "3", "1", "400.0", "300.0", "0.0", "0.75"]
    assert rows[1][3:7] == ["0", "", "-0.7", "0.9"] and rows[1][7:] == ["0", "0", "0.0", "0.0", "0.0", "-1.0"]
    assert rows[3][0] == str(2 ** 40) and rows[3][4] == "" and rows[3][9:] == ["NaN", "inf", "-inf", "NaN"]
    assert rows[4][9:12] == ["9007199254740994.0", "-0.0", "5e-324"]
    assert len(rows) == n and all(len(x) == len(output.PURITY_HEADERS) == 13 for x in rows)
    twin, native = str(tmp_path / "twin.tsv"), str(tmp_path / "native.tsv")
    output.write_purity(twin, rows)
    output.write_purity_native(native, *args)
    assert open(twin, "rb").read() == open(native, "rb").read()
    assert open(native).readline().rstrip("\n").split("\t") == output.PURITY_HEADERS
    # no rows: the header alone, from both
    empty = api.PurityResult(*(np.zeros(0, t) for t in (np.uint32, np.uint32, np.float64, np.float64, np.float64, F)), 0, 0, {})
    none = ([], files, [], [], [], [], np.zeros(0, F), np.zeros(0, F), empty)
    output.write_purity(twin, output.purity_rows(*none))
    output.write_purity_native(native, *none)
    assert open(twin, "rb").read() == open(native, "rb").read()
    # refused: a file id out of range, a null argument
    with pytest.raises(L.SageHipError, match="file id out of range"):
        output.write_purity_native(native, [1], files, [2], ["s"], [2], [""], [0.0], [0.0], api.PurityResult(
            np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1, F), 0, 0, {}))
    assert L.load().sage_hip_write_purity(None, 0, None, None, None, None, None, None, None, None, None, 0) == 1


def world_file(path, w):
    off, mz, it = flatten(w.batches)
    n = len(w.ms1_index)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<QQfffIII", len(off) - 1, n, w.ppm, w.default[0], w.default[1], w.max_isotope, 0 if w.lo is None else 1, 0))
        for a, t in ((off, np.uint64), (mz, F), (it, F), (w.ms1_index, np.uint64), (w.mz, F), (w.charge, np.uint8)):
            fh.write(np.ascontiguousarray(a, t).tobytes())
        if w.lo is not None:
            fh.write(np.ascontiguousarray(w.lo, F).tobytes())
            fh.write(np.ascontiguousarray(w.hi, F).tobytes())
    return path


def test_host_emulation_stand_alone_under_sanitizers(tmp_path):
    """the emulation as a program of its own with AddressSanitizer and UndefinedBehaviorSanitizer, over every named world"""
    exe = str(tmp_path / "purity_emu_san")
    subprocess.check_call(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPURITY_EMU_MAIN",
                           SRC, "-o", exe])
    files = [world_file(str(tmp_path / f"{name}.world"), W.world(name)) for name in W.NAMES]
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"purity_emu ok ({len(files)} worlds)" in r.stdout, r.stdout + r.stderr
