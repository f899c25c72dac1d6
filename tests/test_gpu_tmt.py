"""TMT reporter-ion quantification on the device (sage_hip_tmt, tmt.hip) against the sequential restatement
(tests/tmt_reference.py): the selected peak's intensity AND its index, bit for bit, at level 2 (after the device's own
preprocessing) and at level 3 (raw peaks, no sort), then the command line end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tmt_reference as R
from sage_amd import output
from sage_amd.api import (DatabaseParameters, DeviceDatabase, Isobaric, RawBatch, RawSpectrum, Scorer, ScorerParams,
                          SpectrumProcessor, tmt)
from sage_amd.synthetic import synthetic_fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
TOL = ("ppm", -20.0, 20.0)
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 150, 151, 2047, 2048, 2049, 5000)


def label_sets():
    rng = np.random.default_rng(5)
    t18 = Isobaric("Tmt18").reporter_masses()
    user7 = np.array([131.1, 126.127726, 126.127726, 126.1277, 129.5, 127.1247, 127.1311], dtype=F32)  # unsorted, dup, overlap
    sets = {v: Isobaric(v).reporter_masses() for v in ("Tmt6", "Tmt10", "Tmt11", "Tmt16", "Tmt18")}
    sets.update({"user0": np.zeros(0, F32), "user1": np.array([128.13], F32), "user7": user7,
                 "user300": np.concatenate([rng.choice(t18, 100), rng.uniform(110.0, 150.0, 200)]).astype(F32)})
    return sets


def edge_peaks(labels, rng):
    """m/z exactly on each label's f32 bounds (after the -PROTON offset) and a few ulps either side"""
    mz = []
    for lab in labels[:40]:
        lo, hi = R.bounds(lab, TOL)
        for b in (F32(lo - R.PROTON), F32(hi - R.PROTON)):
            c = F32(b + R.PROTON)
            for k in range(-3, 4):
                x = c
                for _ in range(abs(k)):
                    x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf))
                mz.append(x)
    return np.array(mz, dtype=F32)


def random_spectrum(n, labels, rng, sort=True):
    if n == 0:
        return np.zeros(0, F32), np.zeros(0, F32)
    parts = [rng.uniform(100.0, 2000.0, n)]
    if len(labels):
        parts.append(rng.choice(labels, n) * (1.0 + rng.normal(0.0, 12.0, n) * 1e-6))
        parts.append(edge_peaks(labels, rng))
    mz = np.concatenate(parts).astype(F32)
    mz = mz[rng.permutation(len(mz))[:n]]
    if n > 4:  # equal masses
        mz[rng.integers(0, n, n // 8)] = mz[rng.integers(0, n, n // 8)]
    it = rng.choice([1000.0, 5000.0, 5000.0, 20000.0], n).astype(F32) * rng.integers(1, 4, n).astype(F32)
    special = rng.random(n)
    it[special < 0.03] = np.nan
    it[(special >= 0.03) & (special < 0.05)] = -0.0
    it[(special >= 0.05) & (special < 0.07)] = -50.0
    it[(special >= 0.07) & (special < 0.08)] = np.inf
    it[(special >= 0.08) & (special < 0.10)] = 0.0
    if sort:
        o = np.argsort(mz, kind="stable")
        mz, it = mz[o], it[o]
    return mz, it


def batch(sizes, labels, seed, sort):
    rng = np.random.default_rng(seed)
    spectra = []
    for i, n in enumerate(sizes):
        mz, it = random_spectrum(int(n), labels, rng, sort)
        spectra.append(RawSpectrum(mz, it, float(rng.uniform(400, 1200)), int(rng.integers(0, 4)) or None, id=f"scan={i}"))
    return RawBatch(spectra), spectra


def assert_equal_bits(got_i, got_k, want_i, want_k, what):
    assert np.array_equal(got_k, want_k), (what, np.argwhere(got_k != want_k)[:5])
    assert np.array_equal(got_i.view(np.uint32), want_i.view(np.uint32)), what


@pytest.mark.parametrize("name", list(label_sets()))
def test_level3_raw_peaks_match_restatement(gpu_required, name):
    labels = label_sets()[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    sizes = list(SIZES) + list(rng.integers(0, 700, 60))
    raw, spectra = batch(sizes, labels, seed=len(labels), sort=False)
    res = tmt([raw], labels, 3)
    assert res.intensity.shape == (raw.n, len(labels))
    for i, s in enumerate(spectra):
        m, it, pos = R.process_other_level(s.mz, s.intensity)
        want_i, want_k = R.quantify_spectrum(3, m, it, labels, TOL, raw_position=pos)
        assert_equal_bits(res.intensity[i], res.peak_index[i], want_i, want_k, (name, i, len(s.mz)))


def test_level3_large_spectrum_and_several_batches(gpu_required):
    labels = Isobaric("Tmt18").reporter_masses()
    a, sa = batch([100_000, 3, 0], labels, seed=1, sort=False)
    b, sb = batch([65, 0, 64, 129], labels, seed=2, sort=False)
    res = tmt([a, RawBatch([]), b], labels, 4)
    for i, s in enumerate(sa + sb):
        m, it, pos = R.process_other_level(s.mz, s.intensity)
        want_i, want_k = R.quantify_spectrum(4, m, it, labels, TOL, raw_position=pos)
        assert_equal_bits(res.intensity[i], res.peak_index[i], want_i, want_k, i)


@pytest.fixture(scope="module")
def scorer():
    db = DatabaseParameters(enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P")).build(synthetic_fasta(30, seed=2))
    return Scorer(DeviceDatabase(db, 0), ScorerParams())


@pytest.mark.parametrize("name", ["Tmt6", "Tmt11", "Tmt16", "Tmt18", "user0", "user1", "user7", "user300"])
@pytest.mark.parametrize("deisotope", [True, False])
def test_level2_processed_peaks_match_restatement(gpu_required, scorer, name, deisotope):
    labels = label_sets()[name]
    cutoff = float(R.min_deisotope_mz(labels))
    rng = np.random.default_rng(len(labels) + 7 * deisotope)
    sizes = list(SIZES) + list(rng.integers(0, 400, 40))
    raw, spectra = batch(sizes, labels, seed=3 + len(labels), sort=True)
    top_n = 150
    res = tmt([raw], labels, 2, top_n, deisotope, cutoff)
    proc = SpectrumProcessor(top_n, deisotope, cutoff)
    # the device's processed peaks (min_peaks 0: every spectrum kept) are the host processor's
    dbatch, _ = scorer.process_upload(raw, top_n, deisotope, cutoff, 0)
    off, dm, di, _ = dbatch.download()
    dbatch.close()
    for i, s in enumerate(spectra):
        p = proc.process(s)
        m, it = np.asarray(p.masses, F32), np.asarray(p.intensities, F32)
        a, b = int(off[i]), int(off[i + 1])
        assert np.array_equal(dm[a:b].view(np.uint32), m.view(np.uint32)) and np.array_equal(di[a:b].view(np.uint32), it.view(np.uint32))
        want_i, want_k = R.quantify_spectrum(2, m, it, labels, TOL)
        assert_equal_bits(res.intensity[i], res.peak_index[i], want_i, want_k, (name, i, len(s.mz)))


def test_take_top_n_refused(gpu_required):
    raw, _ = batch([10], Isobaric("Tmt6").reporter_masses(), 0, True)
    with pytest.raises(Exception, match="take_top_n"):
        tmt([raw], Isobaric("Tmt6"), 2, 0)


# ---- command line end to end ---------------------------------------------------------------------------------------------------
def test_cli_tmt_end_to_end(tmp_path):
    from sage_amd.lcms import synthetic_sps_ms3, write_sps
    from sage_amd.mzml import read_mzml
    fasta = tmp_path / "db.fasta"
    fasta.write_text(synthetic_fasta(60, seed=11))
    dbp = {"fasta": str(fasta), "enzyme": {"missed_cleavages": 1, "cleave_at": "KR", "restrict": "P"}, "static_mods": {"C": 57.0215}}
    db = DatabaseParameters.from_json(dbp).build(open(fasta).read())
    labels = Isobaric("Tmt18").reporter_masses()
    paths = write_sps(str(tmp_path / "mzml"), synthetic_sps_ms3(db, labels, n_files=3, ms2_per_file=80, seed=9))
    names = [os.path.basename(p) for p in paths]
    base = {"database": dbp, "precursor_tol": {"ppm": [-10, 10]}, "fragment_tol": {"ppm": [-10, 10]}, "mzml_paths": paths,
            "min_peaks": 10, "min_matched_peaks": 4}
    runs = (("plain", {}, []), ("l3sn", {"quant": {"tmt": "Tmt18", "tmt_settings": {"level": 3, "sn": True}}}, []),
            ("l2", {"quant": {"tmt": "Tmt18", "tmt_settings": {"level": 2}}}, []),
            ("l2host", {"quant": {"tmt": "Tmt18", "tmt_settings": {"level": 2}}}, ["--host-preprocess"]),
            ("l1", {"quant": {"tmt": "Tmt10", "tmt_settings": {"level": 1}}}, []),
            ("user0", {"quant": {"tmt": {"User": []}}}, []))
    outs = {}
    for name, extra, flags in runs:
        cfg = tmp_path / f"{name}.json"
        cfg.write_text(json.dumps(dict(base, **extra)))
        out = tmp_path / name
        subprocess.run([sys.executable, "-m", "sage_amd.cli", str(cfg), "-o", str(out)] + flags, cwd=ROOT, check=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
        outs[name] = out
    plain = (outs["plain"] / "results.sage.tsv").read_bytes()
    assert len(plain.splitlines()) > 40
    assert (outs["l3sn"] / "results.sage.tsv").read_bytes() == plain
    assert (outs["l2"] / "results.sage.tsv").read_bytes() == (outs["l2host"] / "results.sage.tsv").read_bytes()
    paths_of = lambda n: json.load(open(outs[n] / "results.json"))["output_paths"]
    assert paths_of("l3sn") == [str(outs["l3sn"] / "results.sage.tsv"), str(outs["l3sn"] / "tmt.tsv")]
    assert [os.path.basename(p) for p in paths_of("plain")] == ["results.sage.tsv"]
    assert not (outs["l1"] / "tmt.tsv").exists() and not (outs["plain"] / "tmt.tsv").exists()
    assert json.load(open(outs["l1"] / "results.json"))["summary"]["tmt_rows"] == 0

    # level 3 with S/N: the restatement over the Python reader's MS3 spectra
    ids, fids, iit, vals = [], [], [], []
    for fid, p in enumerate(paths):
        for s in read_mzml(p, fid, 3, 3):
            m, it, pos = R.process_other_level(s.mz, s.intensity)
            v, _ = R.quantify_spectrum(3, m, it, labels, TOL, raw_position=pos)
            ids.append(R.row_spec_id(3, s.id, s.precursor_ref)), fids.append(fid), iit.append(s.ion_injection_time), vals.append(v)
    want = tmp_path / "want3.tsv"
    output.write_tmt(str(want), Isobaric("Tmt18").headers(), output.tmt_rows(names, fids, ids, iit, np.array(vals)))
    assert (outs["l3sn"] / "tmt.tsv").read_bytes() == want.read_bytes()
    assert len(ids) == 240 and json.load(open(outs["l3sn"] / "results.json"))["summary"]["tmt_rows"] == 240

    # level 2: every MS2 spectrum, processed with the reporter cut-off, spectrum ids as rows
    proc = SpectrumProcessor(150, True, Isobaric("Tmt18").min_deisotope_mz())
    ids, fids, iit, vals = [], [], [], []
    for fid, p in enumerate(paths):
        for s in read_mzml(p, fid, 2):
            q = proc.process(s)
            v, _ = R.quantify_spectrum(2, np.asarray(q.masses, F32), np.asarray(q.intensities, F32), labels, TOL)
            ids.append(R.row_spec_id(2, s.id, s.precursor_ref)), fids.append(fid), iit.append(s.ion_injection_time), vals.append(v)
    want = tmp_path / "want2.tsv"
    output.write_tmt(str(want), Isobaric("Tmt18").headers(), output.tmt_rows(names, fids, ids, iit, np.array(vals)))
    assert (outs["l2"] / "tmt.tsv").read_bytes() == want.read_bytes() == (outs["l2host"] / "tmt.tsv").read_bytes()

    # {"User": []}: one row per MS3 spectrum, the three leading columns only
    rows = (outs["user0"] / "tmt.tsv").read_text().splitlines()
    assert rows[0] == "filename\tscannr\tion_injection_time" and len(rows) == 241 and all(r.count("\t") == 2 for r in rows)
