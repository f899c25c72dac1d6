"""The roll-up of TMT reporter intensities without a device: sage_amd/csrc/tmt_rollup.h compiled for the host
(tests/hostemu/tmt_rollup_emu.cpp) against the plain restatement (tests/tmt_rollup_reference.py), bit for bit, on the named worlds
(tests/tmt_rollup_worlds.py) and on random ones; the row builder on PSM tables made by hand, the configuration keys, the two
writers and the exported symbols.  (sage_hip_tmt_rollup itself needs a device: tests/test_gpu_tmt_rollup.py.)"""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import tmt_rollup_reference as REF
import tmt_rollup_worlds as W
from sage_amd import _lib as L
from sage_amd import cli, output

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "tmt_rollup_emu.cpp")
LIB = os.path.join(HERE, "hostemu", "libtmt_rollup_emu.so")
CSRC = os.path.join(HERE, "..", "sage_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("tmt_rollup.h", "maxlfq.h", "crlog.h", "crlog_tables.h", "detmath.h")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
dp, up, fp = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
CODE = {"None": 0, "Total": 1, "Sum": 0, "Median": 1}


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
        subprocess.check_call(["g++", "-O2", *FLAGS, "-fPIC", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.emu_tmt_rollup.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, fp, up, dp, dp, up, up, dp, dp,
                                   C.POINTER(C.c_uint64)]
    lib.emu_tmt_rollup.restype = C.c_int
    return lib


def run_emu(lib, w, summary, normalise):
    n, ng = w.n_labels, w.n_groups
    x = np.ascontiguousarray(w.intensity, np.float32)
    g = np.ascontiguousarray(w.group_of_row, np.uint32)
    out = dict(abundance=np.zeros((ng, n)), log_abundance=np.zeros((ng, n)), n_cells=np.zeros((ng, n), np.uint32),
               n_rows_used=np.zeros(ng, np.uint32), factor=np.zeros(n), column_sum=np.zeros(n))
    used = C.c_uint64(0)
    ptr = lambda k, t: out[k].ctypes.data_as(C.POINTER(t))
    rc = lib.emu_tmt_rollup(len(x), n, ng, w.min_present, CODE[normalise], CODE[summary], x.ctypes.data_as(fp), g.ctypes.data_as(up),
                            ptr("abundance", C.c_double), ptr("log_abundance", C.c_double), ptr("n_cells", C.c_uint32),
                            ptr("n_rows_used", C.c_uint32), ptr("factor", C.c_double), ptr("column_sum", C.c_double), C.byref(used))
    assert rc == 0, (w.name, rc)
    out["n_used_rows"] = used.value
    return out


@pytest.mark.parametrize("name", W.NAMES)
def test_host_emulation_equals_the_restatement_on_every_world(emu, name):
    w = W.WORLDS[name]
    for summary, normalise in W.PAIRS:
        W.assert_equal(run_emu(emu, w, summary, normalise), W.reference(name, summary, normalise), (name, summary, normalise), summary)


def test_host_emulation_equals_the_restatement_on_random_worlds(emu):
    for seed in range(200):
        w = W.random_world(seed)
        summary, normalise = W.PAIRS[seed % 4]
        W.assert_equal(run_emu(emu, w, summary, normalise), W.restate(w, summary, normalise), (w.name, summary, normalise), summary)


def test_the_restatement_by_numpy():
    """an independent reading with numpy (tolerances, not bits): sums, factors that equalise the column sums, medians of centred logs"""
    for seed in range(60):
        w = W.random_world(seed)
        x = w.intensity.astype(np.float64)
        ok = W.present(x) & W.used_rows(w)[:, None]
        tot = REF.tmt_rollup(w.intensity.tolist(), w.group_of_row.tolist(), w.n_groups, w.min_present, "Total", "Sum", n_labels=w.n_labels)
        col = np.where(ok, x, 0.0).sum(axis=0)
        assert np.allclose(tot["column_sum"], col, rtol=1e-12)
        some = ok.any(axis=0)
        if some.any():
            f = np.array(tot["factor"])
            assert np.allclose(col[some] * f[some], col[some].mean(), rtol=1e-12) and (f[~some] == 1.0).all()
        med = REF.tmt_rollup(w.intensity.tolist(), w.group_of_row.tolist(), w.n_groups, w.min_present, "None", "Median", n_labels=w.n_labels)
        with np.errstate(all="ignore"):
            logs = np.where(ok, np.log(x), np.nan)
        for g in range(w.n_groups):
            rows = np.flatnonzero((w.group_of_row == g) & W.used_rows(w))
            assert med["n_rows_used"][g] == len(rows)
            want_sum = np.where(ok[rows], x[rows] * np.array(tot["factor"]), 0.0).sum(axis=0)
            assert np.allclose(tot["abundance"][g], want_sum, rtol=1e-12)
            if not len(rows):
                assert all(v != v for v in med["log_abundance"][g])
                continue
            centre = np.nanmean(logs[rows], axis=1)
            d = logs[rows] - centre[:, None]
            for k in range(w.n_labels):
                col_d = d[:, k][~np.isnan(d[:, k])]
                assert med["n_cells"][g][k] == len(col_d)
                if len(col_d):
                    assert abs(med["log_abundance"][g][k] - (np.median(col_d) + centre.mean())) < 1e-9
                    assert abs(med["abundance"][g][k] / np.exp(med["log_abundance"][g][k]) - 1.0) < 1e-12


def test_a_case_worked_by_hand():
    """two channels, rows (1, 3), (3, 1) of one group and (2, 2) of another: column sums 6 and 6, M = 6, factors 1; group 0 sums to
    (4, 4), group 1 to (2, 2).  Median: the centred logs of group 0 are -+ln(3)/2 and +-ln(3)/2, their median 0, so the abundance is
    exp of the mean centre, ln(3)/2: sqrt(3)."""
    got = REF.tmt_rollup([[1.0, 3.0], [3.0, 1.0], [2.0, 2.0]], [0, 0, 1], 2)
    assert got["column_sum"] == [6.0, 6.0] and got["factor"] == [1.0, 1.0] and got["n_rows_used"] == [2, 1]
    assert got["abundance"] == [[4.0, 4.0], [2.0, 2.0]] and got["n_cells"] == [[2, 2], [1, 1]]
    med = REF.tmt_rollup([[1.0, 3.0], [3.0, 1.0], [2.0, 2.0]], [0, 0, 1], 2, summary="Median")
    assert abs(med["abundance"][0][0] - 3.0 ** 0.5) < 1e-15 and abs(med["abundance"][1][1] - 2.0) < 1e-15
    skew = REF.tmt_rollup([[1.0, 3.0], [1.0, 3.0]], [0, 0], 1)   # loading 2 : 6 -> both channels 4
    assert skew["factor"] == [2.0, 4.0 / 6.0] and skew["abundance"][0][0] == 4.0 and abs(skew["abundance"][0][1] - 4.0) < 1e-15


# ---- the row builder: tmt.tsv's rows joined to PSM tables made by hand --------------------------------------------------------------
def _psms(rows):
    """rows: (file_id, scannr, rank, label, peptide_idx, spectrum_q, purity)"""
    f = np.zeros(len(rows), dtype=L.FEATURE_DTYPE)
    for i, r in enumerate(rows):
        f["file_id"][i], f["rank"][i], f["label"][i], f["peptide_idx"][i] = r[0], r[2], r[3], r[4]
    return (f, [r[1] for r in rows], np.array([r[5] for r in rows], np.float32), np.array([r[6] for r in rows], np.float32))


DB = SimpleNamespace(peptide_proteins=lambda i: ["A", "A;B", "B", "A", "C"][i], peptide_info=lambda i: ([1, 2, 1, 1, 1][i], 0),
                     peptide_string=lambda i: ["PEPA", "PEPAB", "PEPB", "PEPA2", "PEPC"][i])


def test_assignment_of_tmt_rows_to_groups():
    q = np.float32(0.01)
    above = float(np.nextafter(q, np.float32(1.0)))
    feats, ids, sq, pur = _psms([(0, "s1", 1, 1, 2, 0.01, 0.9),      # B: exactly at the q-value, kept
                                 (0, "s2", 1, 1, 0, above, 0.9),     # one f32 above it: dropped
                                 (0, "s3", 2, 1, 0, 0.0, 0.9),       # rank 2 only: no PSM
                                 (0, "s4", 1, -1, 0, 0.0, 0.9),      # decoy
                                 (0, "s5", 1, 1, 1, 0.0, 0.9),       # shared peptide (A;B)
                                 (0, "s6", 1, 1, 0, 0.0, -1.0),      # A, purity -1
                                 (0, "s7", 1, 1, 3, 0.0, 0.5),       # A (another peptide), purity exactly min_purity
                                 (1, "s1", 1, 1, 4, 0.0, 0.75),      # C: the same scannr in another file
                                 (0, "s8", 1, 1, 0, 0.0, 0.4999)])   # A, purity below
    tmt_file = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0], np.uint32)
    tmt_ids = ["s7", "s7", "s1", "s2", "s3", "s4", "s5", "s6", "s1", "none", "s8"]   # two MS3 of one MS2 first; an MS3 without PSM
    got, names, pep = output.tmt_rollup_assignment(DB, feats, ids, sq, tmt_file, tmt_ids, None, None, 0.01, None, "protein")
    N = output.NO_GROUP
    assert names == ["A", "B", "C"]
    assert got.tolist() == [0, 0, 1, N, N, N, N, 0, 2, N, 0]
    assert pep.tolist() == [3, 3, 2, -1, -1, -1, -1, 0, 4, -1, 0]
    got, names, _ = output.tmt_rollup_assignment(DB, feats, ids, sq, tmt_file, tmt_ids, None, pur, 0.01, 0.5, "protein")
    assert names == ["A", "B", "C"] and got.tolist() == [0, 0, 1, N, N, N, N, N, 2, N, N]
    got, names, _ = output.tmt_rollup_assignment(DB, feats, ids, sq, tmt_file, tmt_ids, None, None, 0.01, None, "peptide")
    assert names == ["PEPA2", "PEPB", "PEPA", "PEPC"] and got.tolist() == [0, 0, 1, N, N, N, N, 2, 3, N, 2]
    # with protein groups: the group string of the PSM, where it has one group only
    groups = SimpleNamespace(protein_groups=lambda i: ["B", "A/B", "A/B", "A/B", "A/B;C", "A/B", "A/B", "C", "A/B"][i],
                             num_protein_groups=np.array([1, 1, 1, 1, 2, 1, 1, 1, 1], np.uint32))
    got, names, _ = output.tmt_rollup_assignment(DB, feats, ids, sq, tmt_file, tmt_ids, groups, None, 0.01, None, "protein")
    assert names == ["A/B", "B", "C"] and got.tolist() == [0, 0, 1, N, N, N, N, 0, 2, N, 0]


def test_configuration_keys_and_their_refusal():
    defaults = {"by": "protein", "summary": "Sum", "normalise": "Total", "psm_q_value": 0.01, "min_channels": 1, "min_purity": None,
                "plex_of_file": None}
    assert cli.tmt_rollup_settings({}) == (False, defaults)
    assert cli.tmt_rollup_settings({"quant": {"tmt": "Tmt6", "tmt_rollup": False}})[0] is False
    on, st = cli.tmt_rollup_settings({"precursor_purity": True,
                                      "quant": {"tmt": "Tmt18", "tmt_rollup": True,
                                                "tmt_rollup_settings": {"by": "peptide", "summary": "Median", "normalise": "None",
                                                                        "psm_q_value": 0.05, "min_channels": 3, "min_purity": 0.7,
                                                                        "plex_of_file": [0, 0, 1]}}}, 3)
    assert on and st == {"by": "peptide", "summary": "Median", "normalise": "None", "psm_q_value": 0.05, "min_channels": 3,
                         "min_purity": 0.7, "plex_of_file": [0, 0, 1]}
    assert cli.tmt_rollup_settings({"quant": {"tmt": "Tmt6", "tmt_rollup": True, "tmt_rollup_settings": {"summary": None}}})[1] == defaults

    def refused(cfg, *words, n_files=None):
        with pytest.raises(SystemExit) as e:
            cli.tmt_rollup_settings(cfg, n_files)
        assert all(w in str(e.value) for w in words), str(e.value)

    refused({"quant": {"tmt_rollup": True}}, "quant.tmt_rollup", "quant.tmt`")
    refused({"quant": {"tmt": "Tmt6", "tmt_rollup": True, "tmt_rollup_settings": {"min_purity": 0.5}}}, "min_purity", "precursor_purity: true")
    refused({"precursor_purity": False, "quant": {"tmt": "Tmt6", "tmt_rollup": True, "tmt_rollup_settings": {"min_purity": 0.5}}},
            "min_purity", "precursor_purity: true")
    for key, bad in (("by", "gene"), ("summary", "Mean"), ("normalise", "Median")):
        refused({"quant": {"tmt": "Tmt6", "tmt_rollup": True, "tmt_rollup_settings": {key: bad}}},
                f"quant.tmt_rollup_settings.{key}: unknown variant `{bad}`, expected one of")
    refused({"quant": {"tmt": "Tmt6", "tmt_rollup": True, "tmt_rollup_settings": {"plex_of_file": [0, 1]}}}, "plex_of_file", "2 files", "3",
            n_files=3)
    refused({"quant": {"tmt": "Tmt6", "tmt_rollup": True, "tmt_rollup_settings": {"min_channels": -1}}}, "min_channels")


def test_the_two_writers_write_the_same_bytes(tmp_path):
    result = SimpleNamespace(n_rows_used=np.array([3, 0, 1], np.uint32),
                             abundance=np.array([[1.5, 0.0, 1e21], [0.0, 0.0, 0.0], [0.1, 5e-324, 0.0]]))
    second = SimpleNamespace(n_rows_used=np.array([0, 0, 2], np.uint32), abundance=np.array([[0.0] * 3, [0.0] * 3, [7.0, 8.0, 9.0]]))
    ones = np.ones((4, 3), np.float32)
    table = output.tmt_rollup_table([(0, result, np.array([0, 0, 0, 2], np.uint32), np.array([5, 5, 6, 7]), ones),
                                     (4, second, np.array([2, 2, output.NO_GROUP, output.NO_GROUP], np.uint32), np.array([7, 8, -1, -1]), ones)])
    names = ["sp|P1|A;sp|P2|B", "unused", "tab\tname"]
    rows = output.tmt_rollup_rows(names, table)
    assert rows == [["sp|P1|A;sp|P2|B", "0", "3", "2", "1.5", "0.0", "1e21"], ["tab\tname", "0", "1", "1", "0.1", "5e-324", "0.0"],
                    ["tab\tname", "4", "2", "2", "7.0", "8.0", "9.0"]]
    path, native = str(tmp_path / "tmt_proteins.tsv"), str(tmp_path / "native.tsv")
    output.write_tmt_rollup(path, "proteins", ["126", "127N", "a\tb"], rows)
    assert open(path, newline="").read() == ('proteins\tplex\tn_psms\tn_peptides\t126\t127N\t"a\tb"\n'
                                             "sp|P1|A;sp|P2|B\t0\t3\t2\t1.5\t0.0\t1e21\n" '"tab\tname"\t0\t1\t1\t0.1\t5e-324\t0.0\n'
                                             '"tab\tname"\t4\t2\t2\t7.0\t8.0\t9.0\n')
    assert output.write_tmt_rollup_native(native, "proteins", ["126", "127N", "a\tb"], names, table) == 3
    assert open(native, "rb").read() == open(path, "rb").read()
    # no row at all: the header alone, from both
    empty = output.tmt_rollup_table([])
    output.write_tmt_rollup(path, "peptide", ["126"], output.tmt_rollup_rows(names, empty))
    assert output.write_tmt_rollup_native(native, "peptide", ["126"], names, empty) == 0
    assert open(native, "rb").read() == open(path, "rb").read() == b"peptide\tplex\tn_psms\tn_peptides\t126\n"


def test_abi_version_and_exported_symbols():
    lib = L.load()
    assert lib.sage_hip_abi_version() == 6
    new = ["sage_hip_tmt_rollup", "sage_hip_write_tmt_rollup"]
    assert all(s in L.EXPORTED_SYMBOLS for s in new)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(HERE, "..", "include", "sage_hip.h")).read()
    for s in new:
        assert f" T {s}\n" in dynamic, f"{s} is not exported"
        assert f" {s}(" in header, f"{s} is not declared in sage_hip.h"
    assert C.sizeof(L.SageTmtRollupInput) == 48 and C.sizeof(L.SageTmtRollupOutput) == 6 * 8 + 8 + 2 * 4 + 3 * 4 + 4


def test_refusals_that_need_no_device():
    """every status of sage_hip_tmt_rollup is decided before it looks for a device"""
    lib = L.load()
    x = np.ones((2, 3), np.float32)
    g = np.array([0, 5], np.uint32)
    out = dict(ab=np.zeros((2, 3)), la=np.zeros((2, 3)), nc=np.zeros((2, 3), np.uint32), used=np.zeros(2, np.uint32), f=np.zeros(3), s=np.ones(3))
    cout = L.SageTmtRollupOutput(L.as_ptr(out["ab"], C.c_double), L.as_ptr(out["la"], C.c_double), L.as_ptr(out["nc"], C.c_uint32),
                                 L.as_ptr(out["used"], C.c_uint32), L.as_ptr(out["f"], C.c_double), L.as_ptr(out["s"], C.c_double))

    def status(n_rows=2, n_labels=3, n_groups=2, normalise=1, summary=0, intensity=x, groups=g):
        cin = L.SageTmtRollupInput(n_rows, n_labels, n_groups, 1, normalise, summary, None if intensity is None else L.as_ptr(intensity, C.c_float),
                                   None if groups is None else L.as_ptr(groups, C.c_uint32))
        return lib.sage_hip_tmt_rollup(0, C.byref(cin), C.byref(cout)), lib.sage_hip_last_error().decode()

    assert status()[0] == 1 and "group id 5 of row 1" in status()[1]
    assert status(intensity=None)[0] == 1 and "null" in status(intensity=None)[1]
    assert status(groups=None)[0] == 1
    assert status(normalise=2)[0] == 1 and "normalise" in status(normalise=2)[1]
    assert status(summary=-1)[0] == 1 and "summary" in status(summary=-1)[1]
    assert status(n_labels=0)[0] == 1 and "n_labels" in status(n_labels=0)[1]
    assert status(n_labels=65536)[0] == 4 and "65535" in status(n_labels=65536)[1]
    assert status(n_rows=1 << 31)[0] == 4 and "rows" in status(n_rows=1 << 31)[1]
    assert lib.sage_hip_tmt_rollup(0, None, C.byref(cout)) == 1
    # nothing to do: OK without a device.  No group: nothing written; no row, or every row ignored: every group not quantified
    ignored = np.full(2, 0xFFFFFFFF, np.uint32)
    assert status(n_groups=0, groups=ignored)[0] == 0 and out["s"].tolist() == [1.0] * 3
    for rows in (0, 2):
        out["ab"][:], out["la"][:], out["nc"][:], out["used"][:], out["f"][:], out["s"][:] = 9.0, 9.0, 9, 9, 9.0, 9.0
        assert status(n_rows=rows, groups=ignored)[0] == 0
        assert not out["ab"].any() and np.isnan(out["la"]).all() and not out["nc"].any() and not out["used"].any()
        assert out["f"].tolist() == [1.0] * 3 and out["s"].tolist() == [0.0] * 3
        assert cout.n_used_rows == 0 and cout.n_long_groups == 0 and cout.n_label_slabs == 0
