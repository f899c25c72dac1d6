"""MGF input through the command line on the device: the same synthetic spectra written as mzML and as MGF (TITLE = the mzML
id) give the same results.sage.tsv, matched_fragments.sage.tsv and .pin apart from the filename column, with and without the
prefilter pass and with one device named twice; a narrow search leaves spectra annotated with charge 0 without PSM and the
others unchanged."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sage_amd.api import DatabaseParameters, RawSpectrum
from sage_amd.mgf import write_mgf
from sage_amd.mzml import write_mzml
from sage_amd.synthetic import synthetic_fasta, synthetic_spectra

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def spectra(db, n, seed):
    """synthetic MS2 spectra whose retention times survive RTINSECONDS (f32 seconds / 60) bit for bit, peaks ascending"""
    rng = np.random.default_rng(seed)
    out = []
    for i, s in enumerate(synthetic_spectra(db, n, seed=seed)):
        order = np.argsort(np.asarray(s.mz, F32), kind="stable")
        secs = F32(rng.uniform(10, 5000))
        out.append(RawSpectrum(np.asarray(s.mz, F32)[order], np.asarray(s.intensity, F32)[order], float(F32(s.precursor_mz)),
                               s.precursor_charge, None, float(secs / F32(60.0)), id=f"controllerType=0 controllerNumber=1 scan={i + 1}"))
    return out


def run_cli(tmp_path, name, cfg, paths, flags=()):
    p = tmp_path / f"{name}.json"
    p.write_text(json.dumps(dict(cfg, mzml_paths=[str(x) for x in paths])))
    out = tmp_path / name
    subprocess.run([sys.executable, "-m", "sage_amd.cli", str(p), "-o", str(out), *flags], cwd=ROOT, check=True, timeout=600,
                   env=dict(os.environ, PYTHONPATH=ROOT))
    return out


def without_column(text, column):
    rows = [r.split("\t") for r in text.splitlines()]
    k = rows[0].index(column)
    return ["\t".join(r[:k] + r[k + 1:]) for r in rows]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mgf")
    fasta = tmp / "db.fasta"
    fasta.write_text(synthetic_fasta(60, seed=21))
    dbp = {"fasta": str(fasta), "enzyme": {"missed_cleavages": 1, "cleave_at": "KR", "restrict": "P"}, "static_mods": {"C": 57.0215}}
    db = DatabaseParameters.from_json(dbp).build(open(fasta).read())
    files = [spectra(db, 150, seed=31 + k) for k in range(2)]
    return dbp, files


CFG = {"precursor_tol": {"ppm": [-10, 10]}, "fragment_tol": {"ppm": [-10, 10]}, "min_peaks": 10, "min_matched_peaks": 4}


@pytest.mark.parametrize("variant", ["plain", "prefilter", "two_devices"])
def test_mgf_and_mzml_give_the_same_results(world, tmp_path, variant):
    dbp, files = world
    mzml, mgf = [], []
    for k, f in enumerate(files):
        mzml.append(tmp_path / f"run{k}.mzML")
        write_mzml(str(mzml[-1]), f)
        mgf.append(tmp_path / (f"run{k}.mgf" if k == 0 else f"run{k}.mgf.gz"))
        write_mgf(str(mgf[-1]), f)
    cfg = dict(CFG, database=dict(dbp))
    flags = ["--annotate-matches", "--write-pin"]
    if variant == "prefilter":
        cfg["database"] = dict(dbp, prefilter=True, prefilter_chunk_size=20)
    if variant == "two_devices":
        flags += ["--devices", "0,0"]
    a = run_cli(tmp_path, "mzml", cfg, mzml, flags)
    b = run_cli(tmp_path, "mgf", cfg, mgf, flags)
    ta, tb = (a / "results.sage.tsv").read_text(), (b / "results.sage.tsv").read_text()
    assert len(ta.splitlines()) > 50
    assert without_column(ta, "filename") == without_column(tb, "filename")
    assert {r.split("\t")[6] for r in tb.splitlines()[1:]} == {"run0.mgf", "run1.mgf.gz"}
    assert (a / "matched_fragments.sage.tsv").read_bytes() == (b / "matched_fragments.sage.tsv").read_bytes()
    pa, pb = (a / "results.sage.pin").read_text(), (b / "results.sage.pin").read_text()
    assert without_column(pa, "FileName") == without_column(pb, "FileName")


def test_charge_zero_gives_no_psm_in_a_narrow_search(world, tmp_path):
    dbp, files = world
    f = files[0]
    zero = set(range(0, len(f), 5))
    (tmp_path / "with").mkdir()
    (tmp_path / "without").mkdir()
    with_zero = [RawSpectrum(s.mz, s.intensity, s.precursor_mz, 0 if i in zero else s.precursor_charge, None, s.scan_start_time,
                             id=s.id) for i, s in enumerate(f)]
    write_mgf(str(tmp_path / "with" / "run.mgf"), with_zero)
    write_mgf(str(tmp_path / "without" / "run.mgf"), [s for i, s in enumerate(f) if i not in zero])
    cfg = dict(CFG, database=dict(dbp))
    a = run_cli(tmp_path, "with_zero", cfg, [tmp_path / "with" / "run.mgf"])
    b = run_cli(tmp_path, "without_zero", cfg, [tmp_path / "without" / "run.mgf"])
    ta, tb = (a / "results.sage.tsv").read_bytes(), (b / "results.sage.tsv").read_bytes()
    assert len(tb.splitlines()) > 20 and ta == tb
    ids = {r.split("\t")[7] for r in ta.decode().splitlines()[1:]}
    assert not ids & {f[i].id for i in zero}


# ---- ppm isolation windows in the wide-window search (the `_kinds` entry points) ---------------------------------------------
import second_reading as SR  # noqa: E402
from test_scoring_second_reading import F32_FIELDS, F64_FIELDS, INT_FIELDS  # noqa: E402


class KindScorer(SR.SecondScorer):
    """SecondScorer whose wide-window search takes the isolation window as a general Tolerance (kind, lo, hi): mgf.rs:72-83
    gives Tolerance::Ppm for `TOLU=ppm`, and scoring.rs:427-431 scales any kind by the charge (mass.rs:47-57)."""

    def initial_hits(self, masses, prec_mz, prec_charge, isolation):
        if not self.p.wide_window:
            return super().initial_hits(masses, prec_mz, prec_charge, None if isolation is None else isolation[1:])
        mz = SR.f32(prec_mz) - SR.PROTON
        hits = [0, 0, []]
        for z in range(self.p.min_precursor_charge, self.p.max_precursor_charge + 1):
            tol = SR.tol_mul(isolation if isolation is not None else ("da", -2.4, 2.4), SR.f32(z))
            h = self.matched_peaks(masses, mz * SR.f32(z), z, tol)
            hits[0] += h[0]; hits[1] += h[1]; hits[2].extend(h[2])  # noqa: E702
        self.trim_hits(hits)
        return hits


@pytest.fixture(scope="module")
def wide_world(gpu_required):
    import oracle_lib
    from sage_amd.api import DeviceDatabase, ScorerParams, SpectrumBatch, SpectrumProcessor
    dbp = DatabaseParameters(enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"), static_mods={"C": 57.0215})
    host = dbp.build(synthetic_fasta(80, seed=41))
    raws = synthetic_spectra(host, 96, seed=43, isolation_half_width=1.0)
    rng = np.random.default_rng(44)
    kinds = np.where(np.arange(len(raws)) % 2 == 0, 0, 2).astype(np.uint8)  # ppm / Da alternating
    out = []
    for r, k in zip(raws, kinds):
        w = F32(rng.uniform(500.0, 4000.0)) if k == 0 else F32(rng.uniform(0.5, 3.0))  # ppm (0.3-2.5 Da at 600 m/z) or Da
        out.append(RawSpectrum(r.mz, r.intensity, r.precursor_mz, r.precursor_charge, (float(-w), float(w)), r.scan_start_time,
                               id=r.id))
    proc = SpectrumProcessor(150, True, 0.0)
    batch = SpectrumBatch.from_spectra([proc.process(r) for r in out])
    return host, DeviceDatabase(host, 0), oracle_lib.OracleDb.from_product(host), out, kinds, batch, ScorerParams


def test_ppm_wide_window_matches_the_second_reading(wide_world):
    from sage_amd.api import RawBatch, Scorer
    host, dev, orc, raws, kinds, batch, ScorerParams = wide_world
    params = ScorerParams(wide_window=True, report_psms=3, chimera=True)
    scorer = Scorer(dev, params)
    f1, c1 = (a.copy() for a in scorer.score(batch, iso_kind=kinds))
    f2, c2 = (a.copy() for a in scorer.score_resident(scorer.upload(batch, iso_kind=kinds)))
    dbatch, _ = scorer.process_upload(RawBatch(raws), 150, True, 0.0, 0, iso_kind=kinds)
    f3, c3 = (a.copy() for a in scorer.score_resident(dbatch))
    assert np.array_equal(c1, c2) and np.array_equal(c1, c3)
    assert f1.tobytes() == f2.tobytes() == f3.tobytes()
    sr = KindScorer(SR.Peptides(orc.arrays()), [SR.B, SR.Y], 2, params)
    n_psm = 0
    for i in range(batch.n):
        spec = SR.spectrum_of(batch, i)
        spec["isolation"] = ("ppm" if kinds[i] == 0 else "da", batch.isolation_lo[i], batch.isolation_hi[i])
        feats, _ = sr.score(spec)
        assert c1[i] == len(feats), f"spectrum {i}: device {c1[i]} PSMs, second reading {len(feats)}"
        for r, f in enumerate(feats):
            o = f1[i, r]
            for k in INT_FIELDS:
                assert int(o[k]) == int(f[k]), (i, r, k)
            for k in F32_FIELDS:
                assert np.float32(o[k]).view(np.uint32) == np.float32(f[k]).view(np.uint32), (i, r, k)
            for k in F64_FIELDS:
                a, b = float(o[k]), float(f[k])
                assert a == b or abs(a - b) <= 1e-12 * max(abs(b), abs(float(f["hyperscore"])), 1.0), (i, r, k)
            n_psm += 1
    assert n_psm > 50
    # the ppm windows are not the Da windows of the same numbers: the kinds reach the device
    f0, c0 = scorer.score(batch)
    assert not (np.array_equal(c0, c1) and f0.tobytes() == f1.tobytes())


def test_da_windows_through_the_kind_entry_points_are_the_old_entry_points(wide_world):
    from sage_amd.api import RawBatch, Scorer
    host, dev, orc, raws, kinds, batch, ScorerParams = wide_world
    da = np.full(batch.n, 2, np.uint8)
    for params in (ScorerParams(wide_window=True, report_psms=2), ScorerParams(report_psms=2)):
        scorer = Scorer(dev, params)
        for new, old in ((lambda: scorer.score(batch, iso_kind=da), lambda: scorer.score(batch)),
                         (lambda: scorer.score_resident(scorer.upload(batch, iso_kind=da)),
                          lambda: scorer.score_resident(scorer.upload(batch))),
                         (lambda: scorer.score_resident(scorer.process_upload(RawBatch(raws), 150, True, 0.0, 0, iso_kind=da)[0]),
                          lambda: scorer.score_resident(scorer.process_upload(RawBatch(raws), 150, True, 0.0, 0)[0]))):
            fa, ca = (a.copy() for a in new())
            fb, cb = (a.copy() for a in old())
            assert np.array_equal(ca, cb) and fa.tobytes() == fb.tobytes()


# ---- raw peaks in file order: process_kernel<false> / <true> ------------------------------------------------------------------
@pytest.mark.parametrize("deisotope", [True, False], ids=["deisotope", "heap"])
def test_device_processing_of_peaks_in_file_order(wide_world, deisotope):
    import oracle_lib
    import raw_spectra as G
    from sage_amd.api import RawBatch, Scorer, ScorerParams
    dev = wide_world[1]
    rng = np.random.default_rng([91, int(deisotope)])
    raws = []
    for k, n in enumerate([0, 1, 2, 63, 64, 65, 129, 150, 700, 2047, 2048, 2049, 3001, 4097, 10000] + [int(x) for x in rng.integers(3, 1500, 20)]):
        mz, it = G.raw_peaks(rng, n)
        o = rng.permutation(n) if k % 4 else np.arange(n)[::-1]  # shuffled or descending: the order of an MGF file
        raws.append(RawSpectrum(np.ascontiguousarray(mz[o]), np.ascontiguousarray(it[o]), float(F32(rng.uniform(350, 1500))),
                                G.precursor_charge(rng) or None, None, 0.0, id=f"u{k}"))
    scorer = Scorer(dev, ScorerParams())
    min_mz = G.min_deisotope_mz(rng, [r.mz for r in raws])
    dbatch, npk = scorer.process_upload(RawBatch(raws), 150, deisotope, min_mz, 0)
    off, m, it, tic = dbatch.download()
    for i, r in enumerate(raws):
        wm, wi, wt = oracle_lib.process_ms2(150, deisotope, min_mz, r.mz, r.intensity, r.precursor_charge)
        a, b = int(off[i]), int(off[i + 1])
        assert npk[i] == len(wm) == b - a, f"spectrum {i} ({len(r.mz)} raw peaks)"
        np.testing.assert_array_equal(m[a:b].view(np.uint32), np.asarray(wm, F32).view(np.uint32), err_msg=f"spectrum {i}")
        np.testing.assert_array_equal(it[a:b].view(np.uint32), np.asarray(wi, F32).view(np.uint32), err_msg=f"spectrum {i}")
        assert F32(tic[i]) == F32(wt), f"spectrum {i}"
    assert any(len(r.mz) > G.LDS_PEAKS for r in raws)


# ---- TMT level 2 and LFQ on MGF input through the command line ------------------------------------------------------------------
def test_cli_tmt_level2_and_lfq_on_mgf(world, tmp_path):
    import tmt_reference as T
    from sage_amd import output
    from sage_amd.api import Isobaric, SpectrumProcessor
    from sage_amd.mgf import read_mgf_native
    dbp, files = world
    mgf = tmp_path / "run.mgf"
    write_mgf(str(mgf), files[0])
    mzml = tmp_path / "run.mzML"
    write_mzml(str(mzml), files[0])
    cfg = dict(CFG, database=dict(dbp), quant={"tmt": "Tmt18", "tmt_settings": {"level": 2, "sn": True}})
    out = run_cli(tmp_path, "tmt", cfg, [mgf])
    labels = Isobaric("Tmt18").reporter_masses()
    raw = read_mgf_native(str(mgf))[0]
    proc = SpectrumProcessor(150, True, Isobaric("Tmt18").min_deisotope_mz())
    ids, vals = [], []
    for i in range(raw.n):  # every MS2 spectrum, no S/N division (read_mgf takes no S/N level), injection time 0
        q = proc.process(raw.spectrum(i))
        v, _ = T.quantify_spectrum(2, np.asarray(q.masses, F32), np.asarray(q.intensities, F32), labels)
        ids.append(T.row_spec_id(2, raw.ids[i], "")), vals.append(v)
    want = tmp_path / "want.tsv"
    output.write_tmt(str(want), Isobaric("Tmt18").headers(), output.tmt_rows(["run.mgf"], [0] * raw.n, ids, np.zeros(raw.n), np.array(vals)))
    assert (out / "tmt.tsv").read_bytes() == want.read_bytes() and raw.n == 150
    # LFQ: MGF holds no MS1 spectra, so quantification sees none — as an mzML file of the same MS2 spectra and no MS1 does
    cfg = dict(CFG, database=dict(dbp), quant={"lfq": True})
    a, b = run_cli(tmp_path, "lfq_mgf", cfg, [mgf]), run_cli(tmp_path, "lfq_mzml", cfg, [mzml])
    for name in ("results.sage.tsv", "lfq.tsv"):
        pa, pb = a / name, b / name
        assert pa.exists() == pb.exists()
        if pa.exists():
            col = "filename" if name == "results.sage.tsv" else None
            ta, tb = pa.read_text(), pb.read_text()
            if col:
                assert without_column(ta, col) == without_column(tb, col)
            else:
                assert ta.replace("run.mgf", "run.mzML") == tb
