"""sage_hip_lfq on the device against the sequential restatement (tests/lfq_reference.py): a 3-file synthetic run with a
hand-built feature table for every scoring x integration x combine_charge_states setting, a fixture of named edge cases, and
the command line end to end (lfq.tsv; results.sage.tsv unchanged by the `quant` section).

Exact: grid keys, every grid matrix (f64 bits), warps, best RT bin, left / right bounds, areas (bits), q-values, the passing
count.  spectral_angle and score go through acos, the one device transcendental (ocml acos vs libm acos): they are held to
ULPS units in the last place."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import lfq_reference as R
from lfq_traces import features_table, isotopes_of, mz_for_mass as _mz_for_mass, ref_feats, ref_spectra, run_world
from sage_amd.api import (ALIGNMENT_DTYPE, DatabaseParameters, LfqSettings, RawBatch, RawSpectrum, lfq, peptide_compositions)
from sage_amd.lcms import synthetic_lcms, write_lcms
from sage_amd.synthetic import synthetic_fasta

pytestmark = pytest.mark.gpu

ULPS = 8
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def db():
    return DatabaseParameters(enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                              static_mods={"C": 57.0215}).build(synthetic_fasta(60, seed=11))


def ulp_close(a, b, ulps=ULPS):
    if np.isnan(a) and np.isnan(b):
        return True
    return abs(a - b) <= ulps * np.spacing(max(abs(a), abs(b), np.finfo(np.float64).tiny))


def assert_same(dev, ref, grids, passing, n_files):
    keys = [(int(p), int(z), bool(d)) for p, z, d in zip(dev.peptide_idx, dev.charge, dev.decoy)]
    assert keys == sorted(grids), "grid keys"
    worst = 0.0
    for i, k in enumerate(keys):
        np.testing.assert_array_equal(dev.matrix[i].view(np.uint64), grids[k]["matrix"].view(np.uint64), err_msg=f"matrix {k}")
        r = ref[k]
        assert dev.warps[i].tolist() == r["warps"], k
        assert bool(dev.has_peak[i]) == r["peak"], k
        if not r["peak"]:
            continue
        assert (int(dev.peak_rt[i]), int(dev.left[i]), int(dev.right[i])) == (r["rt"], r["left"], r["right"]), k
        np.testing.assert_array_equal(dev.areas[i].view(np.uint64), np.array(r["areas"]).view(np.uint64), err_msg=f"areas {k}")
        assert ulp_close(dev.score[i], r["score"]) and ulp_close(dev.spectral_angle[i], r["spectral_angle"]), \
            (k, dev.score[i], r["score"], dev.spectral_angle[i], r["spectral_angle"])
        worst = max(worst, abs(dev.spectral_angle[i] - r["spectral_angle"]) / np.spacing(abs(r["spectral_angle"]) or 1.0))
        assert dev.q_value[i] == r["q_value"], k
    assert dev.passing == passing
    return worst


# ---- the synthetic run --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(db):
    return run_world(db)


@pytest.mark.parametrize("combine", [True, False])
@pytest.mark.parametrize("integration", R.INTEGRATION)
@pytest.mark.parametrize("scoring", R.SCORING)
def test_lfq_matches_restatement(db, run, scoring, integration, combine):
    st = LfqSettings(peak_scoring=scoring, integration=integration, combine_charge_states=combine)
    settings = R.default_settings(peak_scoring=scoring, integration=integration, combine_charge_states=combine)
    dev = lfq(run["f"], None, run["art"], run["pq"], run["al"], run["batches"], run["carbon"], run["sulfur"], st, (2, 4), debug=True)
    if combine not in run["cache"]:
        fmap = R.build_feature_map(settings, (2, 4), ref_feats(run["f"], run["art"], run["pq"]))
        run["cache"][combine] = (fmap, R.trace(fmap, run["spectra"], run["alignments"], 3, combine, isotopes_of(db)))
    fmap, grids = run["cache"][combine]
    ref, passing, _ = R.quantify(settings, (2, 4), None, None, None, 3, None, grids=grids)
    assert dev.n_windows == len(fmap["ranges"])
    assert len(grids) > 20 and sum(r["peak"] for r in ref.values()) > 10
    print(f"spectral_angle: at most {assert_same(dev, ref, grids, passing, 3):.0f} ulp from the host's acos")


def test_lfq_confidence_order_argument(db, run):
    """`order` permutes the input into confidence order: the same result as passing the permuted table."""
    perm = np.random.default_rng(4).permutation(len(run["f"]))
    inv = np.argsort(perm)
    st = LfqSettings()
    a = lfq(run["f"], None, run["art"], run["pq"], run["al"], run["batches"], run["carbon"], run["sulfur"], st, (2, 4))
    b = lfq(run["f"][perm], inv.astype(np.uint32), run["art"][perm], run["pq"][perm], run["al"], run["batches"], run["carbon"],
            run["sulfur"], st, (2, 4))
    for k in ("peptide_idx", "charge", "decoy", "peak_rt", "q_value"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    np.testing.assert_array_equal(a.areas.view(np.uint64), b.areas.view(np.uint64))


# ---- named edge cases ----------------------------------------------------------------------------------------------------------
def _time_below(r):
    """an f32 spectrum RT s that passes r <= s + RT_TOL but lies below the grid's rt_min = r - RT_TOL: bin 0 by saturation"""
    s = F32(r - R.RT_TOL)
    for _ in range(64):
        s = np.nextafter(s, F32(-np.inf))
        if r <= s + R.RT_TOL and s >= F32(0) and np.floor((s - (r - R.RT_TOL)) / ((R.RT_TOL * F32(2.0)) / F32(100))) < 0:
            return s
        if not (r <= s + R.RT_TOL):
            return None
    return None


@pytest.fixture(scope="module")
def edge(db):
    rng = np.random.default_rng(8)
    pool = rng.permutation(db.n_peptides)
    rows = []
    # filler: > 16 384 windows, so the feature map has two pages
    for p in pool[:930]:
        rows.append((int(p), 1, float(rng.uniform(800, 3000)), int(rng.integers(0, 3)), float(rng.uniform(0.2, 0.8)), 0.0))
    a, b, c = (int(x) for x in pool[930:933])
    rows.append((a, 1, 2400.0, 0, 0.5, 0.0))      # the ±0.1 pair at 50 ppm: z = 2 windows at 1200.0 and 1200.005
    rows.append((b, 1, 2400.01, 1, 0.5, 0.0))
    rows.append((c, 1, 1500.0, 2, 0.004, 0.0))    # decoy RT clamped to 0; reference file 2 has no MS1 spectra
    f, art, pq = features_table(db, rows)
    al = np.zeros(3, ALIGNMENT_DTYPE)
    for i in range(3):
        al[i] = (i, 1.0, 1.0, 0.0)                  # rt = sst exactly
    settings = R.default_settings(ppm_tolerance=50.0)
    fmap = R.build_feature_map(settings, (2, 4), ref_feats(f, art, pq))
    assert len(fmap["min_rts"]) == 2
    ranges = fmap["ranges"]
    spectra = {0: [], 1: []}
    named = {}

    def add(fid, t, masses, ints=None):
        mz = [_mz_for_mass(F32(m)) if not isinstance(m, tuple) else m[0] for m in masses]
        assert all(x is not None for x in mz)
        ints = ints or [1000.0 * (j + 1) for j in range(len(mz))]
        order = np.argsort(np.array(mz, np.float32), kind="stable")
        spectra[fid].append(RawSpectrum(np.array(mz, np.float32)[order], np.array(ints, np.float32)[order], 0.0, None, None,
                                        float(F32(t)), None, fid, f"t={t}"))
    # a peak exactly on mass_lo and one exactly on mass_hi of a filler window, at its rt
    w = next(e for e in ranges if not e["decoy"] and e["isotope"] == 0 and 0.3 < e["rt"] < 0.7)
    add(0, w["rt"], [w["mass_lo"], w["mass_hi"]])
    named["edges"] = w
    # the ±0.1 miss: a peak at 1200.05 lies in both windows; the first one's mass_lo is below mass - 0.1 -> not found
    add(1, F32(0.5), [F32(1200.05)])
    # decoy RT clamped to 0: the decoy window (rt 0) of peptide c at z = 2, isotope 0, seen at rt 0.001
    dec = next(e for e in ranges if e["peptide"] == c and e["decoy"] and e["charge"] == 2 and e["isotope"] == 0)
    assert dec["rt"] == F32(0.0)
    add(0, F32(0.001), [(dec["mass_lo"] + dec["mass_hi"]) / F32(2.0)])
    # spectrum RT on page 1's min_rt, and rt - RT_TOL on it
    m1 = fmap["min_rts"][1]
    pw = next(e for e in ranges[R.BIN_SIZE:] if e["rt"] == m1)
    add(1, m1, [(pw["mass_lo"] + pw["mass_hi"]) / F32(2.0)])
    s = F32(m1 + R.RT_TOL)
    for _ in range(8):
        if F32(s - R.RT_TOL) == m1:
            break
        s = np.nextafter(s, F32(np.inf) if F32(s - R.RT_TOL) < m1 else F32(-np.inf))
    assert F32(s - R.RT_TOL) == m1
    add(1, s, [(pw["mass_lo"] + pw["mass_hi"]) / F32(2.0)])
    # the saturating bin-0 case and bin 99
    for e in ranges:
        if e["decoy"] or e["isotope"] != 1:
            continue
        t = _time_below(e["rt"])
        if t is not None:
            add(0, t, [(e["mass_lo"] + e["mass_hi"]) / F32(2.0)])
            named["bin0"] = e
            break
    assert "bin0" in named
    add(1, w["rt"] + R.RT_TOL, [(w["mass_lo"] + w["mass_hi"]) / F32(2.0)])
    # an MS1 spectrum without peaks
    spectra[0].append(RawSpectrum(np.zeros(0, np.float32), np.zeros(0, np.float32), 0.0, None, None, 0.5, None, 0, "empty"))
    batches = []
    for fid in (0, 1):
        sp = sorted(spectra[fid], key=lambda x: x.scan_start_time)
        batches.append(RawBatch(sp))
    cc, ss = peptide_compositions(db.seq_off, db.seq)
    return dict(f=f, art=art, pq=pq, al=al, batches=batches, carbon=cc, sulfur=ss, fmap=fmap, named=named, pair=(a, b), c=c,
                spectra=ref_spectra(batches), alignments=[tuple(x) for x in al.tolist()])


@pytest.mark.parametrize("combine", [True, False])
def test_lfq_edge_cases(db, edge, combine):
    settings = R.default_settings(ppm_tolerance=50.0, combine_charge_states=combine, spectral_angle=0.0)
    grids = R.trace(edge["fmap"], edge["spectra"], edge["alignments"], 3, combine, isotopes_of(db))
    ref, passing, _ = R.quantify(settings, (2, 4), None, None, None, 3, None, grids=grids)
    dev = lfq(edge["f"], None, edge["art"], edge["pq"], edge["al"], edge["batches"], edge["carbon"], edge["sulfur"],
              LfqSettings(ppm_tolerance=50.0, combine_charge_states=combine, spectral_angle=0.0), (2, 4), debug=True)
    assert dev.n_windows == len(edge["fmap"]["ranges"]) > R.BIN_SIZE
    assert_same(dev, ref, grids, passing, 3)
    a, b = edge["pair"]
    keys = set(grids)
    assert (b, 0 if combine else 2, False) in keys and (a, 0 if combine else 2, False) not in keys  # the ±0.1 miss
    assert (edge["c"], 0 if combine else 2, True) in keys                                             # clamped decoy RT
    e = edge["named"]["bin0"]
    g = grids[(e["peptide"], 0 if combine else e["charge"], False)]["matrix"]
    assert g[0 * 3 + 1, 1] < 0.0                                                                      # interp < 0 in bin 1
    w = edge["named"]["edges"]
    g = grids[(w["peptide"], 0 if combine else w["charge"], False)]["matrix"]
    assert g[1 * 3 + 0, 99] > 0.0                                                                     # bin 99


# ---- command line end to end ---------------------------------------------------------------------------------------------------
def test_cli_lfq_end_to_end(tmp_path, db):
    fasta = tmp_path / "db.fasta"
    fasta.write_text(synthetic_fasta(60, seed=11))
    files = synthetic_lcms(db, n_files=3, n_peptides=150, ms1_per_file=300, seed=6, ms1_noise=40, ms2_per_peptide=2)
    paths = write_lcms(str(tmp_path / "mzml"), files)
    base = {"database": {"fasta": str(fasta), "enzyme": {"missed_cleavages": 1, "cleave_at": "KR", "restrict": "P"},
                         "static_mods": {"C": 57.0215}},
            "precursor_tol": {"ppm": [-10, 10]}, "fragment_tol": {"ppm": [-10, 10]}, "mzml_paths": paths,
            "min_peaks": 10, "min_matched_peaks": 4}
    outs = {}
    # (this small run's picked-peptide FDR passes no peptide at 1 %: "lfq_all" quantifies every target PSM's peptide)
    runs = (("plain", {}), ("quant_off", {"quant": {"lfq": False}}), ("lfq", {"quant": {"lfq": True}}),
            ("lfq_all", {"quant": {"lfq": True, "lfq_settings": {"peptide_q_value": 1.0}}}))
    for name, extra in runs:
        cfg = tmp_path / f"{name}.json"
        cfg.write_text(json.dumps(dict(base, **extra)))
        out = tmp_path / name
        subprocess.run([sys.executable, "-m", "sage_amd.cli", str(cfg), "-o", str(out)], cwd=ROOT, check=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
        outs[name] = out
    plain = (outs["plain"] / "results.sage.tsv").read_bytes()
    for name in ("quant_off", "lfq", "lfq_all"):
        assert (outs[name] / "results.sage.tsv").read_bytes() == plain, name
    assert not (outs["plain"] / "lfq.tsv").exists() and not (outs["quant_off"] / "lfq.tsv").exists()

    # the restatement fed with this run's own features (results.sage.tsv, confidence order) and MS1 spectra
    lines = plain.decode().splitlines()
    head = lines[0].split("\t")
    col = {k: i for i, k in enumerate(head)}
    rows = [l.split("\t") for l in lines[1:]]
    idx_of = {db.peptide_string(i): i for i in range(db.n_peptides)}
    names = [os.path.basename(p) for p in paths]
    feats = dict(peptide_idx=np.array([idx_of[r[col["peptide"]]] for r in rows]), label=np.array([int(r[col["label"]]) for r in rows]),
                 calcmass=np.array([F32(r[col["calcmass"]]) for r in rows]),
                 file_id=np.array([names.index(r[col["filename"]]) for r in rows]),
                 aligned_rt=np.array([F32(r[col["aligned_rt"]]) for r in rows]), peptide_q=np.array([F32(r[col["peptide_q"]]) for r in rows]))
    from sage_amd import output
    from sage_amd.mzml import read_mzml
    spectra = []
    for fid, p in enumerate(paths):
        for s in read_mzml(p, fid, 1):
            m, it = R.process_ms1(s.mz, s.intensity)
            spectra.append((fid, F32(s.scan_start_time), m, it))
    for name, min_rows, q in (("lfq", 0, 0.01), ("lfq_all", 20, 1.0)):
        summary = json.load(open(outs[name] / "results.json"))["summary"]
        assert str(outs[name] / "lfq.tsv") in summary["output_paths"] and summary["stages"]["lfq_ms"] > 0
        alignments = [(a["file_id"], F32(a["max_rt"]), F32(a["slope"]), F32(a["intercept"])) for a in summary["alignments"]]
        ref, passing, _ = R.quantify(R.default_settings(peptide_q_value=q), (2, 4), feats, spectra, alignments, 3, isotopes_of(db))
        got = (outs[name] / "lfq.tsv").read_text().splitlines()
        assert got[0].split("\t") == output.LFQ_HEADERS + names
        want = [k for k in sorted(ref) if not k[2] and ref[k]["peak"]]
        assert len(want) >= min_rows and len(got) - 1 == len(want), name
        for line, k in zip(got[1:], want):
            r = ref[k]
            v = line.split("\t")
            assert v[0] == db.peptide_string(k[0]) and v[1] == "-1" and v[2] == db.peptide_proteins(k[0])
            assert v[3] == output.ryu_f32(r["q_value"]) and v[6:] == [output.ryu_f64(a) for a in r["areas"]]
            assert ulp_close(float(v[4]), r["score"]) and ulp_close(float(v[5]), r["spectral_angle"])
        assert summary["q_precursor"] == passing
