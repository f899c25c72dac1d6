"""Protein-level label-free quantification (MaxLFQ) without a device: sage_amd/csrc/maxlfq.h compiled for the host
(tests/hostemu/maxlfq_emu.cpp) against the plain restatement (tests/protein_lfq_reference.py), bit for bit, on the named worlds
(tests/protein_lfq_worlds.py) and on random ones; the restatement against a constrained least-squares solve; the row builder, the
configuration keys and the exported symbols.  (sage_hip_protein_lfq itself needs a device: tests/test_gpu_protein_lfq.py.)"""
import ctypes as C
import os
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import protein_lfq_reference as REF
import protein_lfq_worlds as W
from sage_amd import _lib as L
from sage_amd import cli, output

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "maxlfq_emu.cpp")
LIB = os.path.join(HERE, "hostemu", "libmaxlfq_emu.so")
CSRC = os.path.join(HERE, "..", "sage_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("maxlfq.h", "crlog.h", "crlog_tables.h", "detmath.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        subprocess.check_call(["g++", "-O2", *FLAGS, "-fPIC", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.emu_protein_lfq.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, dp, up, dp, dp, up, up, up, dp, up]
    lib.emu_protein_lfq.restype = C.c_int
    return lib


def run_emu(lib, w, pair_tables=True):
    n, npr = w.n_files, w.n_proteins
    pairs = n * (n - 1) // 2
    a = np.ascontiguousarray(w.areas, np.float64)
    por = np.ascontiguousarray(w.protein_of_row, np.uint32)
    out = dict(log_abundance=np.zeros((npr, n)), intensity=np.zeros((npr, n)), component=np.zeros((npr, n), np.uint32),
               n_rows_used=np.zeros(npr, np.uint32), n_components=np.zeros(npr, np.uint32),
               pair_median=np.zeros((npr, pairs)), pair_count=np.zeros((npr, pairs), np.uint32))
    ptr = lambda k, t: out[k].ctypes.data_as(C.POINTER(t))
    rc = lib.emu_protein_lfq(len(a), n, npr, w.min_ratio_count, a.ctypes.data_as(dp), por.ctypes.data_as(up), ptr("log_abundance", C.c_double),
                             ptr("intensity", C.c_double), ptr("component", C.c_uint32), ptr("n_rows_used", C.c_uint32),
                             ptr("n_components", C.c_uint32), ptr("pair_median", C.c_double) if pair_tables else None,
                             ptr("pair_count", C.c_uint32) if pair_tables else None)
    assert rc == 0, (w.name, rc)
    return out


@pytest.mark.parametrize("name", W.NAMES)
def test_host_emulation_equals_the_restatement_on_every_world(emu, name):
    w = W.WORLDS[name]
    W.assert_equal(run_emu(emu, w), W.reference(name), name)
    W.assert_equal(run_emu(emu, w, pair_tables=False), W.reference(name), name, pair_tables=False)


def _random_reference(seed):
    w = W.random_world(seed)
    return w, REF.protein_lfq(w.areas.tolist(), w.protein_of_row.tolist(), w.n_proteins, w.min_ratio_count, n_files=w.n_files)


def test_host_emulation_equals_the_restatement_on_random_worlds(emu):
    for seed in range(200):
        w, want = _random_reference(seed)
        W.assert_equal(run_emu(emu, w), want, w.name)


def test_the_restatement_is_maxlfq():
    """An independent reading of the contract: per component, the least-squares solution of x_j - x_k = m_jk over the valid pairs
    under the constraint that the component's mean equals the mean of its observed logs (numpy.linalg.lstsq with the constraint as
    a heavily weighted row is avoided: the constraint is imposed exactly by shifting the minimum-norm solution)."""
    worst = 0.0
    for seed in range(200):
        w, got = _random_reference(seed)
        n = w.n_files
        pairs = REF.pair_list(n)
        for p in range(w.n_proteins):
            rows = w.areas[w.protein_of_row == p]
            logs = np.where(W.present(rows), np.log(np.where(W.present(rows), rows, 1.0)), np.nan)
            comp = np.array(got["component"][p], np.int64)
            la = np.array(got["log_abundance"][p])
            assert np.array_equal(np.isnan(la), comp == REF.NONE)
            for g in sorted(set(comp[comp != REF.NONE].tolist())):
                members = np.flatnonzero(comp == g)
                eq, rhs = [], []
                for q, (j, k) in enumerate(pairs):
                    if got["pair_count"][p][q] >= max(w.min_ratio_count, 1) and comp[j] == g:
                        assert comp[k] == g
                        row = np.zeros(len(members))
                        row[np.searchsorted(members, j)], row[np.searchsorted(members, k)] = 1.0, -1.0
                        eq.append(row)
                        rhs.append(got["pair_median"][p][q])
                x = np.linalg.lstsq(np.array(eq), np.array(rhs), rcond=None)[0] if eq else np.zeros(len(members))
                observed = logs[:, members]
                x = x - x.mean() + np.nanmean(observed)  # the mean constraint (the minimum-norm solution has mean zero)
                worst = max(worst, float(np.max(np.abs(x - la[members]))))
                assert np.allclose(x, la[members], rtol=0.0, atol=1e-9), (seed, p, g, x, la[members])
            # a file outside every component has no observed value in this protein
            assert not W.present(rows[:, comp == REF.NONE]).any()
    print(f"largest gap between the restatement and the constrained least-squares solve: {worst:.3e}")


def test_pair_medians_of_the_restatement_by_numpy():
    for seed in range(50):
        w, got = _random_reference(seed)
        for p in range(w.n_proteins):
            rows = w.areas[w.protein_of_row == p]
            with np.errstate(all="ignore"):
                logs = np.where(W.present(rows), np.log(rows), np.nan)
            for q, (j, k) in enumerate(REF.pair_list(w.n_files)):
                d = logs[:, j] - logs[:, k]
                d = d[~np.isnan(d)]
                assert got["pair_count"][p][q] == len(d)
                if len(d) >= max(w.min_ratio_count, 1):
                    assert abs(got["pair_median"][p][q] - np.median(d)) < 1e-12


def test_a_case_worked_by_hand():
    """two files, areas (e, 1), (e^3, 1): differences 1 and 3, median 2; x = (2, 0) grounded at file 0 -> (0, -2); the observed mean
    is (1 + 3 + 0 + 0) / 4 = 1, the solution's mean -1: log abundances (2, 0)"""
    e1, e3 = float(np.exp(1.0)), float(np.exp(3.0))
    got = REF.protein_lfq([[e1, 1.0], [e3, 1.0]], [0, 0], 1)
    assert got["pair_count"] == [[2]] and abs(got["pair_median"][0][0] - 2.0) < 1e-15
    assert got["component"] == [[0, 0]] and got["n_components"] == [1] and got["n_rows_used"] == [2]
    assert abs(got["log_abundance"][0][0] - 2.0) < 1e-15 and abs(got["log_abundance"][0][1]) < 1e-15
    assert abs(got["intensity"][0][0] - float(np.exp(2.0))) < 1e-14


def test_protein_lfq_rows_against_a_row_written_by_hand(tmp_path):
    result = SimpleNamespace(n_rows_used=np.array([3, 0, 1], np.uint32), n_components=np.array([1, 0, 0], np.uint32),
                             intensity=np.array([[1.5, 0.0, 1e21], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]))
    rows = output.protein_lfq_rows(["sp|P1|A;sp|P2|B", "unused", "tab\tname"], result)
    assert rows == [["sp|P1|A;sp|P2|B", "3", "1", "1.5", "0.0", "1e21"], ["tab\tname", "1", "0", "0.0", "0.0", "0.0"]]
    path = str(tmp_path / "protein_lfq.tsv")
    output.write_protein_lfq(path, ["a.mzML", "b.mzML", "c.mzML"], rows)
    assert open(path, newline="").read() == ("proteins\tn_precursors\tn_components\ta.mzML\tb.mzML\tc.mzML\n"
                                             "sp|P1|A;sp|P2|B\t3\t1\t1.5\t0.0\t1e21\n" '"tab\tname"\t1\t0\t0.0\t0.0\t0.0\n')
    # the native writer: the same bytes (host code, no device)
    full = SimpleNamespace(**result.__dict__, to_c=lambda keep: L.SageProteinLfqOutput(
        None, L.as_ptr(result.intensity, C.c_double), None, L.as_ptr(result.n_rows_used, C.c_uint32), L.as_ptr(result.n_components, C.c_uint32)))
    native = str(tmp_path / "native.tsv")
    assert output.write_protein_lfq_native(native, ["sp|P1|A;sp|P2|B", "unused", "tab\tname"], full, ["a.mzML", "b.mzML", "c.mzML"]) == 2
    assert open(native, "rb").read() == open(path, "rb").read()


def test_configuration_keys_and_their_refusal():
    assert cli.protein_lfq_settings({}) == (False, {"min_ratio_count": 1, "precursor_q_value": 0.05})
    on, st = cli.protein_lfq_settings({"quant": {"lfq": True, "protein_lfq": True,
                                                 "protein_lfq_settings": {"min_ratio_count": 2, "precursor_q_value": 0.01}}})
    assert on and st == {"min_ratio_count": 2, "precursor_q_value": 0.01}
    assert cli.protein_lfq_settings({"quant": {"lfq": True, "protein_lfq": False}})[0] is False
    assert cli.protein_lfq_settings({"quant": {"lfq": True, "protein_lfq_settings": {"min_ratio_count": None}}})[1]["min_ratio_count"] == 1
    for quant in ({"protein_lfq": True}, {"lfq": False, "protein_lfq": True}):
        with pytest.raises(SystemExit) as e:
            cli.protein_lfq_settings({"quant": quant})
        assert "quant.protein_lfq" in str(e.value) and "quant.lfq" in str(e.value)


def test_assignment_of_rows_to_proteins():
    """shared peptides are left out; ids by first appearance in grid order; the protein-group stage's strings when it ran"""
    db = SimpleNamespace(peptide_proteins=lambda i: ["B", "A;B", "A", "B", "C"][i], peptide_info=lambda i: ([1, 2, 1, 1, 1][i], 0))
    lfq = SimpleNamespace(peptide_idx=np.array([0, 1, 2, 3, 4, 2], np.uint32), q_value=np.array([0.01, 0.01, 0.05, 0.2, 0.01, 0.01], np.float32),
                          target_rows=lambda: np.array([0, 1, 2, 3, 5], np.uint64))
    rows, ids, names = output.protein_lfq_assignment(db, lfq, precursor_q_value=0.05)
    assert rows.tolist() == [0, 2, 5] and ids.tolist() == [0, 1, 1] and names == ["B", "A"]
    feats = np.zeros(3, dtype=L.FEATURE_DTYPE)
    feats["peptide_idx"] = [2, 0, 1]
    groups = SimpleNamespace(protein_groups=lambda i: ["A/B", "B", "A/B"][i], num_protein_groups=np.array([1, 1, 2], np.uint32))
    rows, ids, names = output.protein_lfq_assignment(db, lfq, feats, groups, 0.05)
    assert rows.tolist() == [0, 2, 5] and ids.tolist() == [0, 1, 1] and names == ["B", "A/B"]


def test_abi_version_and_exported_symbols():
    lib = L.load()
    assert lib.sage_hip_abi_version() == 6
    new = ["sage_hip_protein_lfq", "sage_hip_write_protein_lfq"]
    assert all(s in L.EXPORTED_SYMBOLS for s in new)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(HERE, "..", "include", "sage_hip.h")).read()
    for s in new:
        assert f" T {s}\n" in dynamic, f"{s} is not exported"
        assert f" {s}(" in header, f"{s} is not declared in sage_hip.h"
    assert C.sizeof(L.SageProteinLfqInput) == 40 and C.sizeof(L.SageProteinLfqOutput) == 7 * 8 + 4 * 4 + 4 + 4


def test_refusals_that_need_no_device():
    """what sage_hip_protein_lfq answers before it looks for a device"""
    lib = L.load()
    cin = L.SageProteinLfqInput(1, 70000, 1, 1, None, None)
    cout = L.SageProteinLfqOutput()
    assert lib.sage_hip_protein_lfq(0, C.byref(cin), C.byref(cout)) == 4 and b"65535" in lib.sage_hip_last_error()
    cin = L.SageProteinLfqInput(1, 2, 1, 1, None, None)
    assert lib.sage_hip_protein_lfq(0, C.byref(cin), C.byref(cout)) == 1 and b"null" in lib.sage_hip_last_error()
    assert lib.sage_hip_protein_lfq(0, None, C.byref(cout)) == 1


def test_host_emulation_stand_alone_under_sanitizers(emu, tmp_path):
    """the emulation as a program of its own with AddressSanitizer and UndefinedBehaviorSanitizer, over every world"""
    exe = str(tmp_path / "maxlfq_emu_san")
    subprocess.check_call(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMAXLFQ_EMU_MAIN",
                           SRC, "-o", exe])
    files = []
    for name, w in W.WORLDS.items():
        path = str(tmp_path / f"{name}.world")
        with open(path, "wb") as fh:
            fh.write(struct.pack("<QIIII", len(w.areas), w.n_files, w.n_proteins, w.min_ratio_count, 0))
            fh.write(np.ascontiguousarray(w.areas, np.float64).tobytes())
            fh.write(np.ascontiguousarray(w.protein_of_row, np.uint32).tobytes())
        files.append(path)
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"maxlfq_emu ok ({len(files)} worlds)" in r.stdout, r.stdout + r.stderr
