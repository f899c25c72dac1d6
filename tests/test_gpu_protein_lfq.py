"""Protein-level label-free quantification on the device (sage_hip_protein_lfq) against the plain restatement
(tests/protein_lfq_reference.py), bit for bit, on the named worlds of tests/protein_lfq_worlds.py; refused input; and a run of the
command line whose protein_lfq.tsv is rebuilt from the run's own lfq.tsv and results.sage.tsv by the restatement."""
import json
import os

import numpy as np
import pytest

import protein_lfq_reference as REF
import protein_lfq_worlds as W
from sage_amd import _lib as L
from sage_amd import api, cli, output
from sage_amd.lcms import synthetic_lcms, write_lcms
from sage_amd.synthetic import synthetic_fasta
from test_gpu_lfq import db  # noqa: F401  (the fixture: the database of the LFQ tests' synthetic runs)

pytestmark = pytest.mark.gpu


def call(w, debug=True, monkeypatch=None):
    if w.workspace_mb is not None:
        monkeypatch.setenv("SAGE_HIP_PLFQ_WORKSPACE_MB", repr(w.workspace_mb))
    r = api.protein_lfq(w.areas, w.protein_of_row, w.n_proteins, w.min_ratio_count, debug=debug)
    return r, {k: getattr(r, k) for k in ("log_abundance", "intensity", "component", "n_rows_used", "n_components", "pair_median",
                                           "pair_count")}


@pytest.mark.parametrize("name", W.NAMES)
def test_device_equals_the_restatement(name, monkeypatch):
    w = W.WORLDS[name]
    want = W.reference(name)
    r, got = call(w, True, monkeypatch)
    W.assert_equal(got, want, name)
    assert r.n_batches >= w.min_batches, (name, r.n_batches)
    if w.n_proteins and len(w.areas):
        assert r.n_batches >= 1 and r.stage_ms["device_ms"] > 0.0
    # without the pair tables; and once more with them: the same bits (no state between calls)
    _, plain = call(w, False, monkeypatch)
    assert plain["pair_median"] is None and plain["pair_count"] is None
    W.assert_equal(plain, want, name, pair_tables=False)
    _, again = call(w, True, monkeypatch)
    for k, v in got.items():
        assert np.array_equal(v.view(np.uint64 if v.dtype == np.float64 else v.dtype), again[k].view(np.uint64 if v.dtype == np.float64 else v.dtype)), (name, k)
    assert np.array_equal(got["log_abundance"].view(np.uint64), plain["log_abundance"].view(np.uint64))
    assert np.array_equal(got["intensity"].view(np.uint64), plain["intensity"].view(np.uint64))


def test_refused_input():
    areas = np.ones((3, 2))
    with pytest.raises(L.SageHipError, match=r"status 1: .*protein id 5 of row 1"):
        api.protein_lfq(areas, [0, 5, 1], 2)
    with pytest.raises(L.SageHipError, match=r"status 1: .*n_proteins"):
        api.protein_lfq(areas, [0, 0, 0], 0)
    with pytest.raises(L.SageHipError, match=r"status 4: .*65535 files"):
        api.protein_lfq(np.ones((1, 65536)), [0], 1)
    # ignored rows only: fine, nothing is quantified
    r = api.protein_lfq(areas, [W.NONE] * 3, 2)
    assert np.isnan(r.log_abundance).all() and not r.intensity.any() and not r.n_rows_used.any() and (r.component == W.NONE).all()


def test_cli_protein_lfq_end_to_end(tmp_path, db):  # noqa: F811
    fasta = tmp_path / "db.fasta"
    fasta.write_text(synthetic_fasta(60, seed=11))
    files = synthetic_lcms(db, n_files=3, n_peptides=150, ms1_per_file=300, seed=6, ms1_noise=40, ms2_per_peptide=2)
    paths = write_lcms(str(tmp_path / "mzml"), files)
    names = [os.path.basename(p) for p in paths]
    # (this small run's picked-peptide FDR passes no peptide at 1 %: every target PSM's peptide is quantified, every row used)
    base = {"database": {"fasta": str(fasta), "enzyme": {"missed_cleavages": 1, "cleave_at": "KR", "restrict": "P"},
                         "static_mods": {"C": 57.0215}},
            "precursor_tol": {"ppm": [-10, 10]}, "fragment_tol": {"ppm": [-10, 10]}, "mzml_paths": paths,
            "min_peaks": 10, "min_matched_peaks": 4}
    quiet = lambda *a, **k: None
    for grouping in (False, True):
        extra = {"protein_grouping": True} if grouping else {}
        tag = "grouped" if grouping else "flat"
        lfq_only = dict(base, **extra, quant={"lfq": True, "lfq_settings": {"peptide_q_value": 1.0}})
        rolled = dict(base, **extra, quant={"lfq": True, "lfq_settings": {"peptide_q_value": 1.0}, "protein_lfq": True,
                                            "protein_lfq_settings": {"min_ratio_count": 2, "precursor_q_value": 1.0}})
        a, b = tmp_path / f"{tag}_lfq", tmp_path / f"{tag}_rolled"
        cli.run(lfq_only, paths, str(a), log=quiet)
        summary = cli.run(rolled, paths, str(b), log=quiet)
        assert not (a / "protein_lfq.tsv").exists()
        for same in ("lfq.tsv", "results.sage.tsv"):
            assert (a / same).read_bytes() == (b / same).read_bytes(), same
        assert str(b / "protein_lfq.tsv") in summary["output_paths"]
        assert summary["protein_lfq_ms"] > 0 and summary["protein_lfq_device_ms"] > 0
        assert json.load(open(b / "results.json"))["summary"]["protein_lfq_rows"] == summary["protein_lfq_rows"]

        # the rows rebuilt from the run's own lfq.tsv (and the groups of its results.sage.tsv) by the restatement
        res = [l.split("\t") for l in (b / "results.sage.tsv").read_text().splitlines()]
        col = {k: i for i, k in enumerate(res[0])}
        of_peptide = {}
        for r in res[1:]:
            of_peptide.setdefault(r[col["peptide"]], (r[col["protein_groups"]], int(r[col["num_protein_groups"]]), int(r[col["num_proteins"]])))
        lfq = [l.split("\t") for l in (b / "lfq.tsv").read_text().splitlines()]
        assert lfq[0] == output.LFQ_HEADERS + names
        areas, ids, table, id_of = [], [], [], {}
        for r in lfq[1:]:
            if not np.float32(r[3]) <= np.float32(1.0):
                continue
            group, n_groups, n_proteins = of_peptide[r[0]]
            protein, count = (group, n_groups) if grouping else (r[2], n_proteins)
            if count != 1:
                continue
            if protein not in id_of:
                id_of[protein] = len(table)
                table.append(protein)
            ids.append(id_of[protein])
            areas.append([float(x) for x in r[6:]])
        assert len(table) >= 10 and len(areas) > len(table), "the run quantifies too little to test the roll-up"
        want = REF.protein_lfq(areas, ids, len(table), 2, n_files=3)
        got = [l.split("\t") for l in (b / "protein_lfq.tsv").read_text().splitlines()]
        assert got[0] == output.PROTEIN_LFQ_HEADERS + names
        assert len(got) - 1 == len(table) == summary["protein_lfq_rows"]
        quantified = 0
        for line, p in zip(got[1:], range(len(table))):
            assert line[:3] == [table[p], str(want["n_rows_used"][p]), str(want["n_components"][p])], (tag, p)
            for text, la, x in zip(line[3:], want["log_abundance"][p], want["intensity"][p]):
                if la != la:
                    assert text == "0.0"
                else:
                    assert REF.ulp_distance(float(text), x) <= 1, (tag, p, text, x)
                    quantified += 1
        assert quantified >= len(table)
        # the Python row builder writes the same bytes as the native writer
        result = api.protein_lfq(np.array(areas), ids, len(table), 2)
        again = tmp_path / f"{tag}_python.tsv"
        output.write_protein_lfq(str(again), names, output.protein_lfq_rows(table, result))
        assert again.read_bytes() == (b / "protein_lfq.tsv").read_bytes()
