"""Precursor purity on the device (sage_hip_precursor_purity) against the plain restatement
(tests/purity_reference.py), every output bit, on the named worlds of tests/purity_worlds.py — which sit on the kernel's seams and
say so in tests/test_purity_cpu.py; every world again through the scan route alone (SAGE_HIP_PURITY_SCAN=1, read in a child
process of its own); and a run of the command line whose purity.sage.tsv is rebuilt by the restatement from the files as the Python
mzML reader reads them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import purity_reference as REF
import purity_worlds as W
from sage_amd import api, cli, output
from sage_amd.api import RawBatch
from sage_amd.lcms import synthetic_lcms, write_lcms
from sage_amd.mzml import read_mzml
from sage_amd.synthetic import synthetic_fasta
from test_gpu_lfq import db  # noqa: F401  (the fixture: the database of the LFQ tests' synthetic runs)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def call(w):
    r = api.precursor_purity(w.batches, w.ms1_index, w.mz, w.charge, w.lo, w.hi, w.ppm, w.max_isotope, w.default)
    return r, {k: getattr(r, k) for k in W.FIELDS}


@pytest.mark.parametrize("name", W.NAMES)
def test_device_equals_the_restatement(name, monkeypatch):
    monkeypatch.delenv("SAGE_HIP_PURITY_SCAN", raising=False)
    w = W.world(name)
    r, got = call(w)
    W.assert_equal(got, W.reference(name), name)
    if w.sorted_spectra is not None:
        assert r.n_sorted_spectra == w.sorted_spectra, (name, r.n_sorted_spectra, r.n_scanned_spectra)
    if w.scanned_spectra is not None:
        assert r.n_scanned_spectra == w.scanned_spectra, (name, r.n_sorted_spectra, r.n_scanned_spectra)
    with_spectrum = np.unique(w.ms1_index[w.ms1_index != REF.NO_MS1])
    assert r.n_sorted_spectra + r.n_scanned_spectra == len(with_spectrum)
    if len(with_spectrum):
        assert r.stage_ms["device_ms"] > 0.0 and r.stage_ms["kernel_ms"] > 0.0
    else:
        assert r.stage_ms == {"upload_ms": 0.0, "kernel_ms": 0.0, "device_ms": 0.0}
    # once more: the same bits (no state between calls)
    _, again = call(w)
    W.assert_equal(again, {k: np.asarray(v) for k, v in got.items()}, name)


def test_the_order_case_on_the_device():
    """[2^53, 1, 1] and [1, 1, 2^53] in position order: 2^53 and 2^53 + 2, on the sorted route and on the scan route"""
    r, got = call(W.world("order_case"))
    assert got["total"].tolist() == [2.0 ** 53, 2.0 ** 53 + 2.0, 2.0 ** 53, 2.0 ** 53 + 2.0]
    assert (r.n_sorted_spectra, r.n_scanned_spectra) == (2, 2)


def scan_child(path):
    """(in the child, SAGE_HIP_PURITY_SCAN=1 set before the library reads it) every named world -> one .npz"""
    out = {}
    for name in W.NAMES:
        r, got = call(W.world(name))
        for k, v in got.items():
            out[f"{name}.{k}"] = v
        out[f"{name}.routes"] = np.array([r.n_sorted_spectra, r.n_scanned_spectra], np.uint64)
    np.savez(path, **out)


def test_every_world_again_through_the_scan_route(tmp_path, monkeypatch):
    path = tmp_path / "scan.npz"
    env = dict(os.environ, SAGE_HIP_PURITY_SCAN="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    subprocess.run([sys.executable, "-c", f"import test_gpu_purity as t; t.scan_child({str(path)!r})"], cwd=ROOT, env=env, check=True,
                   timeout=300)
    got = np.load(path)
    monkeypatch.delenv("SAGE_HIP_PURITY_SCAN", raising=False)
    sorted_here = 0
    for name in W.NAMES:
        w = W.world(name)
        W.assert_equal({k: got[f"{name}.{k}"] for k in W.FIELDS}, W.reference(name), f"{name} (scan route)")
        here, _ = call(w)
        n_sorted, n_scanned = (int(x) for x in got[f"{name}.routes"])
        assert n_sorted == 0 and n_scanned == here.n_sorted_spectra + here.n_scanned_spectra, name
        sorted_here += here.n_sorted_spectra
    assert sorted_here >= 40, "the routes did not differ between the two runs"


def test_refused_input_and_empty_calls():
    w = W.world("nan_mz")
    with pytest.raises(api.L.SageHipError, match=r"status 1: .*ms1_index"):
        api.precursor_purity(w.batches, [3], [500.0], [2])
    with pytest.raises(api.L.SageHipError, match=r"status 1: .*max_isotope"):
        api.precursor_purity(w.batches, [0], [500.0], [2], max_isotope=17)
    r = api.precursor_purity(w.batches, [], [], [])
    assert len(r.purity) == 0 and r.n_sorted_spectra == r.n_scanned_spectra == 0


def test_cli_precursor_purity_end_to_end(tmp_path, db):  # noqa: F811
    fasta = tmp_path / "db.fasta"
    fasta.write_text(synthetic_fasta(60, seed=11))
    files = synthetic_lcms(db, n_files=2, n_peptides=80, ms1_per_file=120, seed=9, ms1_noise=40, ms2_per_peptide=2)
    for lf in files:  # isolation offsets on two of every three MS2 scans; the others fall back to the default pair
        k = 0
        for s, level in zip(lf.spectra, lf.ms_levels):
            if level == 2:
                k += 1
                if k % 3:
                    s.isolation_window = (-0.4 - 0.1 * (k % 5), 0.6 + 0.2 * (k % 4))
    paths = write_lcms(str(tmp_path / "mzml"), files)
    names = [os.path.basename(p) for p in paths]
    base = {"database": {"fasta": str(fasta), "enzyme": {"missed_cleavages": 1, "cleave_at": "KR", "restrict": "P"},
                         "static_mods": {"C": 57.0215}},
            "precursor_tol": {"ppm": [-10, 10]}, "fragment_tol": {"ppm": [-10, 10]}, "mzml_paths": paths,
            "min_peaks": 10, "min_matched_peaks": 4, "report_psms": 2}
    settings = {"ppm_tolerance": 8.0, "max_isotope": 3, "default_isolation": [-0.6, 0.9]}
    quiet = lambda *a, **k: None
    a, b = tmp_path / "plain", tmp_path / "purity"
    plain = cli.run(base, paths, str(a), log=quiet)
    lines = []
    summary = cli.run(dict(base, precursor_purity=True, purity_settings=settings), paths, str(b), log=lambda *x, **k: lines.append(x[0]))
    assert not (a / "purity.sage.tsv").exists() and "purity_rows" not in plain
    assert (a / "results.sage.tsv").read_bytes() == (b / "results.sage.tsv").read_bytes()
    assert str(b / "purity.sage.tsv") in summary["output_paths"] and summary["purity_ms"] > 0
    assert json.load(open(b / "results.json"))["summary"]["purity_rows"] == summary["purity_rows"]
    assert sum("precursor purity" in l and f"({summary['purity_rows']} PSMs" in l for l in lines) == 1

    # one row per reported PSM, in results.sage.tsv's order; the rows rebuilt by the restatement from the Python reader's spectra
    res = [l.split("\t") for l in (b / "results.sage.tsv").read_text().splitlines()]
    col = {k: i for i, k in enumerate(res[0])}
    got = [l.split("\t") for l in (b / "purity.sage.tsv").read_text().splitlines()]
    assert got[0] == output.PURITY_HEADERS and len(got) == len(res) == summary["purity_rows"] + 1 and len(res) > 100
    ms2 = [{s.id: s for s in read_mzml(p, f, 2)} for f, p in enumerate(paths)]
    ms1 = [RawBatch(read_mzml(p, f, 1)) for f, p in enumerate(paths)]
    ms1_ids = [s for m in ms1 for s in m.ids]
    rows = res[1:]
    fid = [names.index(r[col["filename"]]) for r in rows]
    spectra = [ms2[f][r[col["scannr"]]] for f, r in zip(fid, rows)]
    charge = [int(r[col["charge"]]) for r in rows]
    nan = float("nan")
    lo = np.array([s.isolation_window[0] if s.isolation_window else nan for s in spectra], F)
    hi = np.array([s.isolation_window[1] if s.isolation_window else nan for s in spectra], F)
    index = REF.assign_ms1(ms1, fid, [s.scan_start_time for s in spectra])
    want = REF.run(ms1, index, [s.precursor_mz for s in spectra], charge, lo, hi, 8.0, 3, (-0.6, 0.9))
    given = ~np.isnan(lo)
    assert given.sum() > 30 and (~given).sum() > 30 and (index != REF.NO_MS1).sum() > 100
    assert (want["n_matched"] >= 2).sum() > 50 and (want["purity"] > 0.5).sum() > 50, "the run's precursors are not found in its MS1 scans"
    from types import SimpleNamespace
    want_rows = output.purity_rows([int(r[col["psm_id"]]) for r in rows], names, fid, [r[col["scannr"]] for r in rows], charge,
                                   ["" if int(k) == REF.NO_MS1 else ms1_ids[int(k)] for k in index], np.where(given, lo, F(-0.6)),
                                   np.where(given, hi, F(0.9)), SimpleNamespace(**want))
    assert got[1:] == want_rows
