"""Hostile peak lists (tests/hostile_peaks.py) on the device, from raw peaks to PSMs: unsorted and descending m/z, NaN / infinite /
zero / negative m/z and intensities, both infinities in one spectrum (the class in which additions create NaNs), every m/z a NaN;
precursors of NaN, +-inf, 0, -500, 3e38 and PROTON.

  a. process_kernel<false> / <true> against the oracle's SpectrumProcessor::process: masses and intensities BIT FOR BIT (for a
     NaN: NaN-ness and sign — f32::total_cmp orders by it, and the order decides what the top-N cut keeps); the total ion current
     by bits when finite and by NaN-ness otherwise.
  b. the device-processed batch scored (score_resident) against the oracle scoring the oracle-processed spectra; the same
     processed spectra through upload / score (host arrays); once through test_gpu_parity.check with the stream and probe variants.
  c. one MGF file with peak lines out of order and `inf` / `nan` / negative values through the command line, device and host
     preprocessing: byte-identical results, the oracle's PSM count.

tests/test_hostile_peaks_cpu.py has held the host restatement and the readers' emulation to the same lists, and
tests/test_scoring_second_reading.py the oracle to the second reading, so the expected values do not rest on one reading.  The
census of the batches (profiles/hostile_peaks_census.json, held to a fresh one on the CPU) is asserted before any comparison."""
import json

import numpy as np
import pytest

import hostile_peaks as H
import oracle_lib
import raw_spectra as G
from parity_utils import assert_features_equal
from sage_amd.api import (DatabaseParameters, DeviceDatabase, RawBatch, RawSpectrum, Scorer, ScorerParams, SpectrumBatch,
                          SpectrumProcessor)
from test_gpu_parity import check

pytestmark = pytest.mark.gpu
F32 = np.float32
SETTINGS = sorted(H.scorer_settings())


@pytest.fixture(scope="module")
def world(gpu_required):
    with open(H.CENSUS_FILE) as f:
        H.assert_census(json.load(f))
    host = DatabaseParameters(**H.TRYPTIC).build(H.fasta_text())
    return host, DeviceDatabase(host, 0), oracle_lib.OracleDb.from_product(host)


def assert_same_bits(got, want, context):
    gm, gi, gt = got
    wm, wi, wt = want
    assert len(gm) == len(wm), f"{context}: {len(gm)} peaks vs oracle {len(wm)}"
    for name, a, b in (("masses", gm, wm), ("intensities", gi, wi)):
        a, b = H.bits(a), H.bits(b)
        if not np.array_equal(a, b):
            k = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{context}: {name}[{k}] = {a[k]:#010x} vs oracle {b[k]:#010x} ({int((a != b).sum())} of {len(a)} differ)")
    gt, wt = F32(gt), F32(wt)
    assert (np.isnan(gt) and np.isnan(wt)) or H.bits(gt)[0] == H.bits(wt)[0], f"{context}: total ion current {gt!r} vs oracle {wt!r}"


# ---- a. preprocessing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deisotope", [True, False], ids=["deisotope", "heap"])
@pytest.mark.parametrize("cls", H.CLASSES)
def test_device_processing_of_hostile_peaks(world, cls, deisotope):
    _, dev, _ = world
    spectra, top_n, min_mz, min_peaks = H.preprocessing_batch(cls, deisotope)
    raws = [RawSpectrum(mz, it, 600.0, z or None, None, float(k), None, 0, f"{cls}{k}") for k, (mz, it, z) in enumerate(spectra)]
    assert any(len(r.mz) > G.LDS_PEAKS for r in raws) and any(len(r.mz) <= G.LDS_PEAKS for r in raws)   # both instances run
    ctx = f"{cls}, deisotope={deisotope} take_top_n={top_n} min_deisotope_mz={min_mz!r} min_peaks={min_peaks}"
    scorer = Scorer(dev, ScorerParams())
    dbatch, npk = scorer.process_upload(RawBatch(raws), take_top_n=top_n, deisotope=deisotope, min_deisotope_mz=min_mz,
                                        min_peaks=min_peaks)
    off, m, it, tic = dbatch.download()
    created, first_error = set(), None
    for i, r in enumerate(raws):
        w = oracle_lib.process_ms2(top_n, deisotope, min_mz, r.mz, r.intensity, r.precursor_charge)
        c = f"{ctx}: spectrum {i} ({len(r.mz)} raw peaks)"
        assert npk[i] == len(w[0]), f"{c}: out_npeaks {npk[i]} vs oracle {len(w[0])}"
        a, b = int(off[i]), int(off[i + 1])
        if len(w[0]) < min_peaks:
            assert b == a, f"{c}: {b - a} peaks in the batch below min_peaks"
            continue
        if cls == "both_inf":  # no NaN goes in: every NaN that comes out was made by an addition
            created |= {f"intensity {x:#010x}" for x in H.bits(it[a:b])[np.isnan(it[a:b])]}
            created |= {f"tic {x:#010x}" for x in H.bits(tic[i:i + 1])[np.isnan(tic[i:i + 1])]}
        try:
            assert_same_bits((m[a:b], it[a:b], tic[i]), w, c)
        except AssertionError as e:  # (the whole batch's created NaNs are printed before the first difference is raised)
            first_error = first_error or e
    if cls == "both_inf":
        print(f"hostile_peaks: {ctx}: NaNs created on the device (inf + -inf): {sorted(created)}")
        assert created, "no addition created a NaN"
    if first_error:
        raise first_error
    scorer.close()


# ---- b. scoring ---------------------------------------------------------------------------------------------------------------------
def _score_three_ways(dev, orc, params, raws, deisotope, min_peaks, ctx):
    """process_upload + score_resident, and the oracle-processed spectra through upload + score_resident and through score: all
    against the oracle.  Returns (oracle counts per raw spectrum, the oracle-processed batch of the kept spectra)."""
    scorer = Scorer(dev, params)
    dbatch, npk = scorer.process_upload(RawBatch(raws), take_top_n=150, deisotope=deisotope, min_deisotope_mz=0.0, min_peaks=min_peaks)
    gf, gc = (a.copy() for a in scorer.score_resident(dbatch))
    want = H.oracle_processed(raws, 150, deisotope)
    kept = [i for i, w in enumerate(want) if len(w.masses) >= min_peaks]
    assert [int(x) for x in npk] == [len(w.masses) for w in want], f"{ctx}: out_npeaks"
    hb = SpectrumBatch.from_spectra([want[i] for i in kept])
    of, oc, _, _ = orc.score(params, hb)
    dropped = np.setdiff1d(np.arange(len(raws)), kept)
    assert np.all(gc[dropped] == 0), f"{ctx}: PSMs for spectra below min_peaks"
    sub_f, sub_c = gf[kept].copy(), gc[kept]
    sub_f["spec_index"] = np.where(np.arange(sub_f.shape[1])[None, :] < sub_c[:, None], np.arange(len(kept))[:, None], sub_f["spec_index"])
    n = assert_features_equal(sub_f, sub_c, of, oc, f"{ctx}: device-processed batch")
    assert n == int(oc.sum())
    g2, c2 = (a.copy() for a in scorer.score_resident(scorer.upload(hb)))
    assert_features_equal(g2, c2, of, oc, f"{ctx}: host arrays, upload + score_resident")
    g3, c3 = scorer.score(hb)
    assert_features_equal(g3, c3, of, oc, f"{ctx}: host arrays, score")
    scorer.close()
    full = np.zeros(len(raws), np.int64)
    full[kept] = oc
    return full, hb


@pytest.mark.parametrize("mode", ["deisotope", "heap"])
@pytest.mark.parametrize("name", SETTINGS)
def test_device_scoring_of_hostile_peaks(world, name, mode):
    host, dev, orc = world
    kw, chimeric, annotated = H.scorer_settings()[name]
    raws, _ = H.peak_spectra(host, chimeric)
    if not annotated:
        for r in raws:
            r.precursor_charge = None
    oc, hb = _score_three_ways(dev, orc, ScorerParams(**kw), raws, mode == "deisotope", 15 if mode == "deisotope" else 0,
                               f"hostile peaks, {name}, {mode}")
    assert (oc > 0).sum() >= H.MIN_PEAK_FRACTION * len(raws), f"{name}, {mode}: {(oc > 0).sum()} of {len(raws)} spectra have a PSM"
    assert np.isnan(hb.masses).any() and np.isinf(hb.masses).any() and (hb.masses < 0).any() and np.isnan(hb.total_ion_current).any()


@pytest.mark.parametrize("name", SETTINGS)
def test_device_scoring_of_hostile_precursors(world, name):
    host, dev, orc = world
    kw, _, annotated = H.scorer_settings()[name]
    raws, touched = H.precursor_spectra(host, annotated)
    oc, _ = _score_three_ways(dev, orc, ScorerParams(**kw), raws, True, 0, f"hostile precursors, {name}")
    assert (oc[~touched] > 0).sum() >= H.MIN_PRECURSOR_FRACTION * (~touched).sum(), f"{name}: {oc[~touched]}"


@pytest.mark.parametrize("variant", ["stream", "probe"])
def test_narrow_variants_on_hostile_batches(world, monkeypatch, variant):
    """the preliminary lists (heap order included), every Feature field, a second step on the handle and score_batch, with the
    narrow kernel walking the peptide-major list (stream) and reading the tiles' succinct tables (probe)"""
    host, dev, orc = world
    monkeypatch.setenv("SAGE_HIP_NARROW", variant)
    settings = H.scorer_settings()
    raws, _ = H.peak_spectra(host)
    praws, _ = H.precursor_spectra(host)
    n = 0
    for deisotope in (True, False):
        batch = SpectrumBatch.from_spectra(H.oracle_processed(raws, 150, deisotope))
        for name in ("narrow", "da3_report5", "isotope_errors"):
            n += check(dev, orc, batch, ScorerParams(**settings[name][0]), f"{variant}: hostile peaks, {name}, deisotope={deisotope}")[0]
    pbatch = SpectrumBatch.from_spectra(H.oracle_processed(praws))
    for name in ("narrow", "da3_report5", "isotope_errors"):
        n += check(dev, orc, pbatch, ScorerParams(**settings[name][0]), f"{variant}: hostile precursors, {name}")[0]
    assert n > 300


# ---- c. one MGF file through the command line ---------------------------------------------------------------------------------------
def _as_an_mgf_file_can_hold(raws):
    """A peak line starts with a digit (mgf.rs:276-299): a line whose m/z is spelled `nan`, `-inf` or `-300` is no peak line.  What
    a file CAN hold in the m/z column is an unsigned decimal — 0, 3e38, and `1e39`, which f32::from_str rounds to +inf.  The
    m/z values no file can hold become +inf; the intensity column takes every spelling."""
    out = []
    for r in raws:
        mz = np.where(np.isnan(r.mz) | np.signbit(r.mz), F32(np.inf), r.mz).astype(F32)
        out.append(RawSpectrum(mz, r.intensity, r.precursor_mz, r.precursor_charge, None, r.scan_start_time, None, 0, r.id))
    return out


def _mgf_text(raws):
    """BEGIN IONS blocks with the peak lines in the order given; non-finite values in the spellings f32::from_str takes"""
    spell = {"inf": ["inf", "Infinity", "+inf", "INF"], "-inf": ["-inf", "-Infinity"], "nan": ["nan", "NaN"]}
    out = []
    for k, r in enumerate(raws):
        def text(x):
            x = F32(x)
            if np.isnan(x):
                return ("-" if np.signbit(x) else "") + spell["nan"][k % 2]
            if np.isinf(x):
                return spell["inf" if x > 0 else "-inf"][k % len(spell["inf" if x > 0 else "-inf"])]
            return repr(float(x)) if x != 0 else ("-0" if np.signbit(x) else "0")
        lines = ["BEGIN IONS", f"TITLE={r.id}", f"RTINSECONDS={k + 1}", f"PEPMASS={float(F32(r.precursor_mz))!r}", f"CHARGE={r.precursor_charge}+"]
        lines += [f"{'1e39' if np.isinf(m) else text(m)} {text(i)}" for m, i in zip(r.mz, r.intensity)]
        out.append("\n".join(lines + ["END IONS"]) + "\n")
    return "".join(out)


def test_cli_on_an_mgf_file_of_hostile_peaks(world, tmp_path):
    from sage_amd import cli
    from sage_amd.mgf import read_mgf_native
    host, dev, orc = world
    raws, names = H.peak_spectra(host)
    raws = _as_an_mgf_file_can_hold(raws)
    fasta = tmp_path / "db.fasta"
    fasta.write_text(H.fasta_text())
    mgf = tmp_path / "hostile.mgf"
    mgf.write_text(_mgf_text(raws))
    cfg = dict(database=dict(H.TRYPTIC, fasta=str(fasta)), precursor_tol={"ppm": [-10, 10]}, fragment_tol={"ppm": [-10, 10]},
               deisotope=True, min_peaks=15, report_psms=2, min_matched_peaks=3)
    quiet = lambda *a, **k: None  # noqa: E731
    cli.run(cfg, [str(mgf)], str(tmp_path / "device"), log=quiet)
    cli.run(cfg, [str(mgf)], str(tmp_path / "host"), log=quiet, host_preprocess=True)
    a = (tmp_path / "device" / "results.sage.tsv").read_bytes()
    b = (tmp_path / "host" / "results.sage.tsv").read_bytes()
    assert a == b, "results.sage.tsv differs between device and host preprocessing"
    # what the reader made of the file is what was written (bits, file order), and the oracle's PSM count on the restated spectra
    raw = read_mgf_native(str(mgf))[0]
    assert raw.n == len(raws)
    for i, r in enumerate(raws):
        s = raw.spectrum(i)
        assert np.array_equal(H.bits(s.mz), H.bits(r.mz)) and np.array_equal(H.bits(s.intensity), H.bits(r.intensity)), f"spectrum {i} ({names[i]})"
    sp = cli.search_parameters(cfg)
    proc = SpectrumProcessor(sp["max_peaks"], sp["deisotope"], 0.0)
    kept = [p for p in (proc.process(raw.spectrum(i)) for i in range(raw.n)) if len(p.masses) >= sp["min_peaks"]]
    _, oc, _, _ = orc.score(cli.scorer_params(sp), SpectrumBatch.from_spectra(kept))
    rows = a.decode().splitlines()[1:]
    assert len(rows) == int(oc.sum()) and (oc > 0).sum() >= H.MIN_PEAK_FRACTION * len(raws), (len(rows), int(oc.sum()))
