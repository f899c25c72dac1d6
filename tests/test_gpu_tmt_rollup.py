"""The roll-up of TMT reporter intensities on the device (sage_hip_tmt_rollup) against the plain restatement
(tests/tmt_rollup_reference.py), bit for bit, on the named worlds of tests/tmt_rollup_worlds.py for the four (summary, normalise)
pairs; refused input; and runs of the command line whose tmt_proteins.tsv is rebuilt by the restatement from the run's own tmt.tsv,
results.sage.tsv and purity.sage.tsv."""
import json
import os

import numpy as np
import pytest

import tmt_rollup_reference as REF
import tmt_rollup_worlds as W
from sage_amd import _lib as L
from sage_amd import api, cli, output
from sage_amd.api import DatabaseParameters, Isobaric
from sage_amd.synthetic import synthetic_fasta

pytestmark = pytest.mark.gpu
KEYS = ("abundance", "log_abundance", "n_cells", "n_rows_used", "factor", "column_sum", "n_used_rows")
# The q-value bound of the end-to-end runs.  Runs this small pass no peptide at 1 % (the picked FDR over ~120 spectra has few decoys
# to count with), so the runs take every PSM up to 0.5; rebuilt_table() asserts that the bound keeps at least 5 proteins.
PSM_Q = 0.5


def call(w, summary, normalise):
    r = api.tmt_rollup(w.intensity, w.group_of_row, w.n_groups, w.min_present, normalise, summary)
    return r, {k: getattr(r, k) for k in KEYS}


@pytest.mark.parametrize("name", W.NAMES)
def test_device_equals_the_restatement(name):
    w = W.WORLDS[name]
    for summary, normalise in W.PAIRS:
        what = (name, summary, normalise)
        r, got = call(w, summary, normalise)
        W.assert_equal(got, W.reference(name, summary, normalise), what, summary)
        if got["n_used_rows"]:
            assert r.stage_ms["device_ms"] > 0.0 and r.n_label_slabs == (w.n_labels + 63) // 64, what
        else:
            assert r.n_label_slabs == 0 and r.n_long_groups == 0, what
        assert r.n_long_groups >= (w.long_groups if summary == "Median" else 0), what
        _, again = call(w, summary, normalise)   # the same bits (no state between calls, nothing that depends on arrival order)
        for k in KEYS[:-1]:
            a, b = np.asarray(got[k]), np.asarray(again[k])
            view = np.uint64 if a.dtype == np.float64 else a.dtype
            assert np.array_equal(a.view(view), b.view(view)), (what, k)


def test_refused_input():
    x = np.ones((3, 2), np.float32)
    with pytest.raises(L.SageHipError, match=r"status 1: .*group id 5 of row 1 is not below n_groups"):
        api.tmt_rollup(x, [0, 5, 1], 2)
    with pytest.raises(L.SageHipError, match=r"status 1: .*group id 0 of row 0 is not below n_groups"):
        api.tmt_rollup(x, [0, 0, 0], 0)
    with pytest.raises(L.SageHipError, match=r"status 1: .*n_labels == 0"):
        api.tmt_rollup(np.ones((3, 0), np.float32), [0, 0, 0], 1)
    with pytest.raises(L.SageHipError, match=r"status 4: .*65535 channels"):
        api.tmt_rollup(np.ones((1, 65536), np.float32), [0], 1)
    with pytest.raises(ValueError, match="normalise: unknown variant `Median`"):
        api.tmt_rollup(x, [0, 0, 0], 1, normalise="Median")
    with pytest.raises(ValueError, match="summary: unknown variant `Mean`"):
        api.tmt_rollup(x, [0, 0, 0], 1, summary="Mean")
    lib = L.load()
    for field, value, word in (("normalise", 2, b"normalise 2"), ("summary", 7, b"summary 7")):
        cin = L.SageTmtRollupInput(0, 0, 0, 1, 1, 0, None, None)
        setattr(cin, field, value)
        assert lib.sage_hip_tmt_rollup(0, L.C.byref(cin), L.C.byref(L.SageTmtRollupOutput())) == 1 and word in lib.sage_hip_last_error()
    # ignored rows only, or no row that min_present keeps: fine, nothing is quantified
    for groups, need in (([W.NONE] * 3, 1), ([0, 1, 1], 3)):
        r = api.tmt_rollup(x, groups, 2, min_present=need)
        assert np.isnan(r.log_abundance).all() and not r.abundance.any() and not r.n_rows_used.any() and not r.n_cells.any()
        assert r.factor.tolist() == [1.0, 1.0] and r.column_sum.tolist() == [0.0, 0.0] and r.n_used_rows == 0


# ---- command line end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sps(tmp_path_factory):
    """2 SPS-MS3 files of 60 MS2 each; every MS2 also carries a cluster of reporter peaks, so the runs quantify at level 2 too"""
    from sage_amd.lcms import synthetic_sps_ms3, write_sps
    root = tmp_path_factory.mktemp("tmt_rollup")
    fasta = root / "db.fasta"
    fasta.write_text(synthetic_fasta(60, seed=11))
    dbp = {"fasta": str(fasta), "enzyme": {"missed_cleavages": 1, "cleave_at": "KR", "restrict": "P"}, "static_mods": {"C": 57.0215}}
    db = DatabaseParameters.from_json(dbp).build(open(fasta).read())
    labels = Isobaric("Tmt18").reporter_masses()
    files = synthetic_sps_ms3(db, labels, n_files=2, ms2_per_file=60, seed=9)
    rng = np.random.default_rng(21)
    for sf in files:
        for s, level in zip(sf.spectra, sf.ms_levels):
            if level != 2:
                continue
            keep = rng.random(len(labels)) < 0.85
            mz = np.concatenate([s.mz, (labels[keep] * (1.0 + rng.normal(0.0, 3.0, keep.sum()) * 1e-6)).astype(np.float32)])
            it = np.concatenate([s.intensity, rng.lognormal(float(np.log(np.median(s.intensity))), 0.7, keep.sum()).astype(np.float32)])
            o = np.argsort(mz, kind="stable")
            s.mz, s.intensity = mz[o], it[o]
    paths = write_sps(str(root / "mzml"), files)
    base = {"database": dbp, "precursor_tol": {"ppm": [-10, 10]}, "fragment_tol": {"ppm": [-10, 10]}, "mzml_paths": paths,
            "min_peaks": 10, "min_matched_peaks": 4}
    return root, base, paths


def table_of(path):
    lines = [l.split("\t") for l in open(path, newline="").read().split("\n")[:-1]]
    return lines[0], lines[1:]


def rebuilt_table(out, by_groups, settings, headers):
    """tmt_proteins.tsv's text rows by the restatement, from the files the run wrote"""
    head, res = table_of(out / "results.sage.tsv")
    col = {k: i for i, k in enumerate(head)}
    purity = {}
    if settings.get("min_purity") is not None:
        ph, prow = table_of(out / "purity.sage.tsv")
        purity = {int(r[ph.index("psm_id")]): np.float32(r[ph.index("purity")]) for r in prow}
    first = {}   # (filename, scannr) -> the rank-1 target PSM of the smallest psm_id (the first in the order they were scored)
    for r in res:
        if r[col["rank"]] == "1" and r[col["label"]] == "1":
            key = (r[col["filename"]], r[col["scannr"]])
            if key not in first or int(r[col["psm_id"]]) < int(first[key][col["psm_id"]]):
                first[key] = r
    th, rows = table_of(out / "tmt.tsv")
    assert th == output.TMT_HEADERS + headers
    filenames = sorted({r[0] for r in rows})
    plex_of = dict(zip(filenames, settings.get("plex_of_file") or [0] * len(filenames)))
    ids, names, id_of, peptide, dropped_by_purity = [], [], {}, [], 0
    for r in rows:
        ids.append(REF.NONE)
        peptide.append(None)
        p = first.get((r[0], r[1]))
        if p is None or not np.float32(p[col["spectrum_q"]]) <= np.float32(settings["psm_q_value"]):
            continue
        if purity and not purity[int(p[col["psm_id"]])] >= np.float32(settings["min_purity"]):
            dropped_by_purity += 1
            continue
        name, count = (p[col["protein_groups"]], p[col["num_protein_groups"]]) if by_groups else (p[col["proteins"]], p[col["num_proteins"]])
        if count != "1":
            continue
        ids[-1], peptide[-1] = id_of.setdefault(name, len(id_of)), p[col["peptide"]]
        if len(names) < len(id_of):
            names.append(name)
    x = [[float(np.float32(v)) for v in r[3:]] for r in rows]
    need = max(settings.get("min_channels", 1), 1)
    text, values = [], []
    per_plex = {}
    for plex in sorted(set(plex_of.values())):
        at = [i for i, r in enumerate(rows) if plex_of[r[0]] == plex]
        per_plex[plex] = (at, REF.tmt_rollup([x[i] for i in at], [ids[i] for i in at], len(names), need, settings.get("normalise", "Total"),
                                             settings.get("summary", "Sum"), n_labels=len(headers)))
    for g in range(len(names)):
        for plex, (at, want) in per_plex.items():
            if not want["n_rows_used"][g]:
                continue
            peps = {peptide[i] for i in at if ids[i] == g and sum(1 for v in x[i] if REF.present(v)) >= need}
            text.append([names[g], str(plex), str(want["n_rows_used"][g]), str(len(peps))])
            values.append(want["abundance"][g])
    return names, text, values, ids, dropped_by_purity


def run_pair(sps, tag, extra, tmt_level, settings):
    root, base, paths = sps
    quiet = lambda *a, **k: None
    quant = {"tmt": "Tmt18", "tmt_settings": {"level": tmt_level}}
    a, b = root / f"{tag}_plain", root / f"{tag}_rolled"
    cli.run(dict(base, **extra, quant=quant), paths, str(a), log=quiet)
    lines = []
    summary = cli.run(dict(base, **extra, quant=dict(quant, tmt_rollup=True, tmt_rollup_settings=settings)), paths, str(b),
                      log=lambda *x, **k: lines.append(x[0]))
    assert not (a / "tmt_proteins.tsv").exists()
    for same in ("tmt.tsv", "results.sage.tsv"):
        assert (a / same).read_bytes() == (b / same).read_bytes(), same
    assert str(b / "tmt_proteins.tsv") in summary["output_paths"] and summary["tmt_rollup_ms"] > 0
    assert json.load(open(b / "results.json"))["summary"]["tmt_rollup_rows"] == summary["tmt_rollup_rows"]
    assert any("TMT roll-up" in l for l in lines)
    return b, summary


@pytest.mark.parametrize("level", [3, 2])
@pytest.mark.parametrize("grouping", [False, True])
def test_cli_tmt_rollup_end_to_end(sps, level, grouping):
    headers = Isobaric("Tmt18").headers()
    settings = {"psm_q_value": PSM_Q, "min_channels": 2}
    b, summary = run_pair(sps, f"l{level}_{'grouped' if grouping else 'flat'}", {"protein_grouping": True} if grouping else {}, level, settings)
    names, text, values, ids, _ = rebuilt_table(b, grouping, settings, headers)
    print(f"level {level}, grouping {grouping}: {len(names)} proteins from {sum(i != REF.NONE for i in ids)} of {len(ids)} spectra")
    assert len(names) >= 5, "the run quantifies too little to test the roll-up"
    assert len(ids) == 120 and any(i == REF.NONE for i in ids)
    want = b.parent / f"{b.name}_want.tsv"
    output.write_tmt_rollup(str(want), "proteins", headers, [t + [output.ryu_f64(np.float64(v)) for v in vs] for t, vs in zip(text, values)])
    assert (b / "tmt_proteins.tsv").read_bytes() == want.read_bytes()
    assert summary["tmt_rollup_rows"] == len(text) >= 5
    assert any(v > 0.0 for vs in values for v in vs)


def test_cli_tmt_rollup_with_purity_plexes_and_median(sps):
    """min_purity drops some PSMs and keeps others; the two files as two plexes; Median without normalisation, by peptide"""
    headers = Isobaric("Tmt18").headers()
    settings = {"psm_q_value": PSM_Q, "min_purity": 0.0, "plex_of_file": [3, 1], "summary": "Median", "normalise": "None"}
    # (the files' MS1 scans are 50 random peaks: a window of +-10 Da holds a peak for about half of the precursors, purity 0.0 or
    # more; the others have purity -1.0)
    extra = {"precursor_purity": True, "purity_settings": {"default_isolation": [-10.0, 10.0]}}
    b, summary = run_pair(sps, "purity", extra, 3, settings)
    names, text, values, ids, dropped = rebuilt_table(b, False, settings, headers)
    kept = sum(i != REF.NONE for i in ids)
    print(f"purity: {len(names)} proteins, {kept} spectra kept, {dropped} dropped by min_purity")
    assert dropped > 0 and kept > 0 and len(names) >= 5
    head, got = table_of(b / "tmt_proteins.tsv")
    assert head == ["proteins"] + output.TMT_ROLLUP_HEADERS + headers
    assert [r[:4] for r in got] == text and {r[1] for r in got} == {"1", "3"}
    for r, vs in zip(got, values):
        for t, v in zip(r[4:], vs):
            assert (t == "0.0" and v == 0.0) or REF.ulp_distance(float(t), v) <= 1, (r[:2], t, v)
    # by peptide: another file name and first column, the groups are the modified sequences
    root, base, paths = sps
    c = root / "by_peptide"
    cfg = dict(base, quant={"tmt": "Tmt18", "tmt_rollup": True, "tmt_rollup_settings": {"by": "peptide", "psm_q_value": PSM_Q}})
    s2 = cli.run(cfg, paths, str(c), log=lambda *a, **k: None)
    head, got = table_of(c / "tmt_peptides.tsv")
    assert head[0] == "peptide" and not (c / "tmt_proteins.tsv").exists() and s2["tmt_rollup_rows"] == len(got) >= 5
    assert all(r[3] == "1" for r in got)
