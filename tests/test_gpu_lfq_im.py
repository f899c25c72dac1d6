"""sage_hip_lfq_im on the device against the sequential restatement (tests/lfq_im_reference.py), with the contract of
sage_hip_lfq (tests/test_gpu_lfq.py) unchanged.

Exact: grid keys, every grid matrix (f64 bits), warps, best RT bin, left / right bounds, areas (bits), q-values, the passing
count.  spectral_angle and score go through the device's acos and are held to the ULPS of test_gpu_lfq.py.

A 3-file synthetic run with an ion-mobility dimension for every scoring x integration x combine_charge_states setting (one file
all mobility, one mixed, one without); a fixture of named edge cases at tolerance 1 % and 0; two metamorphic identities that
need no oracle; two isobaric co-eluting peptides that only the mobility window tells apart; the command line end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lfq_im_reference as RI
import lfq_reference as R
from sage_amd.api import ALIGNMENT_DTYPE, DatabaseParameters, LfqSettings, RawBatch, RawSpectrum, lfq, lfq_im, peptide_compositions
from sage_amd.lcms import synthetic_ion_mobility, synthetic_lcms, write_lcms
from sage_amd.synthetic import synthetic_fasta
from test_gpu_lfq import ULPS, _mz_for_mass, assert_same, features_table, isotopes_of, ulp_close

pytestmark = pytest.mark.gpu

assert ULPS == 8
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULT_ARRAYS = ("peptide_idx", "charge", "decoy", "has_peak", "peak_rt", "left", "right", "score", "spectral_angle", "q_value",
                 "areas", "warps", "matrix")


@pytest.fixture(scope="module")
def db():
    return DatabaseParameters(enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                              static_mods={"C": 57.0215}).build(synthetic_fasta(60, seed=11))


def ref_feats(f, art, pq):
    return dict(peptide_idx=f["peptide_idx"], label=f["label"], calcmass=f["calcmass"], file_id=f["file_id"], aligned_rt=art,
                peptide_q=pq, ims=f["ims"])


def ref_spectra(batches):
    out = []
    for b in batches:
        for i in range(b.n):
            lo, hi = int(b.peak_off[i]), int(b.peak_off[i + 1])
            if b.mobility is not None and b.has_mobility[i]:
                m, it, mob = RI.process_ms1(b.mz[lo:hi], b.intensities[lo:hi], b.mobility[lo:hi])
            else:
                (m, it), mob = R.process_ms1(b.mz[lo:hi], b.intensities[lo:hi]), None
            out.append((int(b.file_id[i]), F32(b.scan_start_time[i]), m, it, mob))
    return out


def assert_identical(a, b):
    """two device results, every array bit for bit"""
    assert (a.n_windows, a.n_contributions, a.passing) == (b.n_windows, b.n_contributions, b.passing)
    for k in RESULT_ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def unit_alignments(n):
    al = np.zeros(n, ALIGNMENT_DTYPE)
    for i in range(n):
        al[i] = (i, 1.0, 1.0, 0.0)  # rt = scan start time exactly
    return al


# ---- the synthetic run --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(db):
    rng = np.random.default_rng(31)
    files = synthetic_lcms(db, n_files=3, n_peptides=30, ms1_per_file=400, seed=2, ms1_noise=40)
    k0, mobility = synthetic_ion_mobility(db, files, seed=5)
    peps, apex = files[0].peptides, files[0].apex
    rows = []
    for k, p in enumerate(peps):
        fid = k % 3
        if k % 4 == 0:  # a more confident PSM above the threshold, with another mobility: skipped, the next one counts
            rows.append((int(p), 1, float(db.pep_mono[p]), fid, float(apex[k]) + 0.01, 0.5))
        rows.append((int(p), 1, float(db.pep_mono[p]), fid, float(apex[k] + rng.normal(0, 0.0003)), 0.001 * (k % 9)))
        if k % 5 == 0:  # a later confident PSM of the same peptide: ignored, its mobility too
            rows.append((int(p), 1, float(db.pep_mono[p]), (fid + 1) % 3, float(apex[k]) + 0.002, 0.0))
    f, art, pq = features_table(db, rows)
    of = {int(p): k for k, p in enumerate(peps)}
    counted = (pq <= F32(0.01))
    first = {}
    for i in range(len(f)):
        p = int(f[i]["peptide_idx"])
        if counted[i] and p not in first:
            first[p] = i
            f[i]["ims"] = k0[of[p]] * F32(1.0 + rng.uniform(-0.002, 0.002))
        else:
            f[i]["ims"] = F32(5.0)
    # a peptide identified in a spectrum without precursor mobility (ims == 0: window [0, 0]) and one with a NaN
    f[first[int(peps[3])]]["ims"] = 0.0
    f[first[int(peps[7])]]["ims"] = np.nan
    T = 60.0
    al = np.zeros(3, ALIGNMENT_DTYPE)
    for i, lf in enumerate(files):
        al[i] = (i, F32(T), F32(1.0 / lf.rt_scale), F32(-lf.rt_shift / (T * lf.rt_scale)))
    batches = []
    for i, lf in enumerate(files):
        ms1 = [(s, m) for s, m, lvl in zip(lf.spectra, mobility[i], lf.ms_levels) if lvl == 1]
        for j, (s, m) in enumerate(ms1):
            # file 0: every spectrum with mobility; file 1: two of three; file 2: none (no column in the batch)
            s.mobility = m if i == 0 or (i == 1 and j % 3) else None
        if i == 0:
            ms1.insert(10, (RawSpectrum(np.zeros(0, np.float32), np.zeros(0, np.float32), 0.0, None, None, ms1[10][0].scan_start_time,
                                        None, 0, "empty", mobility=np.zeros(0, np.float32)), None))
        batches.append(RawBatch([s for s, _ in ms1]))
    assert batches[0].has_mobility.all() and 0 < batches[1].has_mobility.sum() < batches[1].n and batches[2].mobility is None
    c, s = peptide_compositions(db.seq_off, db.seq)
    return dict(f=f, art=art, pq=pq, al=al, batches=batches, carbon=c, sulfur=s, spectra=ref_spectra(batches),
                alignments=[tuple(a) for a in al.tolist()], cache={})


@pytest.mark.parametrize("combine", [True, False])
@pytest.mark.parametrize("integration", R.INTEGRATION)
@pytest.mark.parametrize("scoring", R.SCORING)
def test_lfq_im_matches_restatement(db, run, scoring, integration, combine):
    st = LfqSettings(peak_scoring=scoring, integration=integration, combine_charge_states=combine)
    settings = R.default_settings(peak_scoring=scoring, integration=integration, combine_charge_states=combine)
    dev = lfq_im(run["f"], None, run["art"], run["pq"], run["al"], run["batches"], run["carbon"], run["sulfur"], st, (2, 4), debug=True)
    if combine not in run["cache"]:
        fmap = RI.build_feature_map(settings, (2, 4), ref_feats(run["f"], run["art"], run["pq"]))
        grids = RI.trace(fmap, run["spectra"], run["alignments"], 3, combine, isotopes_of(db))
        # what the mobility windows removed: the same run traced without the column
        plain = R.trace(fmap, [s[:4] for s in run["spectra"]], run["alignments"], 3, combine, isotopes_of(db))
        run["cache"][combine] = (fmap, grids, plain)
    fmap, grids, plain = run["cache"][combine]
    ref, passing, _ = R.quantify(settings, (2, 4), None, None, None, 3, None, grids=grids)
    assert dev.n_windows == len(fmap["ranges"])
    assert len(grids) > 20 and sum(r["peak"] for r in ref.values()) > 10
    total = lambda g: sum(float(np.abs(v["matrix"]).sum()) for v in g.values())
    assert total(grids) < 0.95 * total(plain), "the mobility windows must remove a visible part of the signal"
    print(f"spectral_angle: at most {assert_same(dev, ref, grids, passing, 3):.0f} ulp from the host's acos")


# ---- named edge cases ----------------------------------------------------------------------------------------------------------
def _edge(db, tol):
    """Five peptides at one RT, masses 200 Da apart; every peak sits in the middle of its peptide's z = 2 monoisotopic window and
    is told apart by its intensity (powers of two per peptide and file: a row's sum names its contributors)."""
    rng = np.random.default_rng(12)
    a, b, c, d, e = (int(x) for x in rng.permutation(db.n_peptides)[:5])
    ims = {a: F32(0.9137), b: F32(0.0), c: F32(-1.0), d: F32(np.nan), e: F32(1.2345)}
    rows = [(p, 1, 1000.0 + 400.0 * k, k % 2, 0.5, 0.0) for k, p in enumerate((a, b, c, d, e))]
    f, art, pq = features_table(db, rows)
    for i, p in enumerate((a, b, c, d, e)):
        f[i]["ims"] = ims[p]
    settings = R.default_settings(ppm_tolerance=20.0, mobility_pct_tolerance=tol, spectral_angle=0.0)
    fmap = RI.build_feature_map(settings, (2, 3), ref_feats(f, art, pq))
    win = {p: next(w for w in fmap["ranges"] if w["peptide"] == p and not w["decoy"] and w["charge"] == 2 and w["isotope"] == 0)
           for p in (a, b, c, d, e)}
    mz = {p: _mz_for_mass(F32((w["mass_lo"] + w["mass_hi"]) / F32(2.0))) for p, w in win.items()}
    assert all(v is not None for v in mz.values())
    lo, hi = win[a]["mobility_lo"], win[a]["mobility_hi"]
    assert (lo, hi) == RI.tol_bounds_pct(ims[a], tol) and (lo < ims[a] < hi if tol else lo == hi == ims[a])
    below, above = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
    expected, power, arrivals = {}, {}, [0]   # (peptide, file) -> the summed intensity that must arrive
    spectra = []

    def spectrum(fid, peaks, with_mobility=True, t=0.5):
        """peaks: (peptide, mobility, arrives).  In the order given (equal m/z keep it through the stable sort)."""
        mzs, its, mobs = [], [], []
        for p, m, arrives in peaks:
            it = float(2 ** power.get((p, fid), 0))
            power[(p, fid)] = power.get((p, fid), 0) + 1
            mzs.append(mz[p]), its.append(it), mobs.append(m)
            expected.setdefault((p, fid), 0.0)
            if arrives:
                expected[(p, fid)] += it
                arrivals[0] += 1
        spectra.append(RawSpectrum(np.array(mzs, np.float32), np.array(its, np.float32), 0.0, None, None, float(F32(t)), None, fid,
                                   f"edge{len(spectra)}", mobility=np.array(mobs, np.float32) if with_mobility else None))
    # exactly on both f32 bounds, and one ulp outside
    spectrum(0, [(a, lo, True), (a, hi, True), (a, below, False), (a, above, False), (a, ims[a], True)])
    # ims == 0: the window [0, 0] takes +0.0 and -0.0 and nothing else
    spectrum(1, [(b, F32(0.0), True), (b, F32(-0.0), True), (b, F32(1e-30), False), (b, F32(-1e-30), False), (b, F32(0.9), False)])
    # negative ims: lo > hi, nothing lies inside; NaN ims: no comparison holds
    clo, chi = win[c]["mobility_lo"], win[c]["mobility_hi"]
    spectrum(0, [(c, F32(-1.0), tol == 0.0), (c, clo, tol == 0.0), (c, chi, tol == 0.0), (c, F32(1.0), False), (d, F32(np.nan), False),
                 (d, F32(0.0), False), (d, F32(1.0), False)])
    # NaN mobilities match no window
    spectrum(1, [(a, F32(np.nan), False), (b, F32(np.nan), False), (e, F32(np.nan), False), (e, ims[e], True)])
    # a spectrum without mobility in the same batch: mass_lookup, whatever the window
    spectrum(0, [(a, F32(9.0), True), (b, F32(9.0), True), (c, F32(9.0), True), (d, F32(9.0), True), (e, F32(9.0), True)], with_mobility=False)
    # equal masses, different mobilities: the stable sort keeps (intensity, mobility) pairs in the order given
    spectrum(1, [(e, F32(0.5), False), (e, ims[e], True), (e, F32(2.0), False), (e, ims[e], True), (e, F32(0.5), False)])
    spectrum(0, [(e, ims[e], True), (e, F32(0.5), False), (e, ims[e], True)])
    assert max(power.values()) <= 12
    # a spectrum above 2 048 peaks: runs of equal m/z (two peptides' windows) with mobilities inside and outside, among noise
    # peaks above every window
    n_big = 3000
    bm = rng.uniform(1600.0, 1900.0, n_big).astype(np.float32)
    bm[rng.choice(n_big, 400, replace=False)] = mz[a]
    bm[rng.choice(np.flatnonzero(bm != mz[a]), 400, replace=False)] = mz[e]
    bmob = rng.uniform(0.5, 1.5, n_big).astype(np.float32)
    inside = rng.random(n_big) < 0.5
    bmob[(bm == mz[a]) & inside] = ims[a]
    bmob[(bm == mz[e]) & inside] = ims[e]
    spectra.append(RawSpectrum(bm, rng.lognormal(8.0, 1.0, n_big).astype(np.float32), 0.0, None, None, float(F32(0.5005)), None, 1,
                               "big", mobility=bmob))
    for p in (a, e):
        w = win[p]
        arrivals[0] += int(((bm == mz[p]) & (bmob >= w["mobility_lo"]) & (bmob <= w["mobility_hi"])).sum())
    batches = [RawBatch([s for s in spectra if s.file_id == fid]) for fid in (0, 1)]
    assert batches[0].has_mobility.tolist() == [1, 1, 0, 1] and max(np.diff(batches[1].peak_off.astype(np.int64))) > 2048
    cc, ss = peptide_compositions(db.seq_off, db.seq)
    al = unit_alignments(2)
    return dict(f=f, art=art, pq=pq, al=al, batches=batches, carbon=cc, sulfur=ss, fmap=fmap, expected=expected, arrivals=arrivals[0],
                peptides=(a, b, c, d, e), settings=settings, spectra=ref_spectra(batches), alignments=[tuple(x) for x in al.tolist()])


@pytest.mark.parametrize("combine", [True, False])
@pytest.mark.parametrize("tol", [1.0, 0.0])
def test_lfq_im_edge_cases(db, tol, combine):
    ed = _edge(db, tol)
    settings = dict(ed["settings"], combine_charge_states=combine)
    grids = RI.trace(ed["fmap"], ed["spectra"], ed["alignments"], 2, combine, isotopes_of(db))
    ref, passing, _ = R.quantify(settings, (2, 3), None, None, None, 2, None, grids=grids)
    dev = lfq_im(ed["f"], None, ed["art"], ed["pq"], ed["al"], ed["batches"], ed["carbon"], ed["sulfur"],
                 LfqSettings(ppm_tolerance=20.0, mobility_pct_tolerance=tol, combine_charge_states=combine, spectral_angle=0.0), (2, 3),
                 debug=True)
    assert_same(dev, ref, grids, passing, 2)
    # the restatement itself against the cases as named: every (peptide, file) row of the monoisotopic z = 2 window sums to the
    # intensities that were to arrive (the 3 000-peak spectrum adds to peptides a and e in file 1), and the device counted
    # exactly the arrivals
    a, b, c, d, e = ed["peptides"]
    for (p, fid), want in ed["expected"].items():
        if fid == 1 and p in (a, e):
            continue
        k = (p, 0 if combine else 2, False)
        got = grids[k]["matrix"][fid * 3 + 0].sum() if k in grids else 0.0
        assert np.isclose(got, want, rtol=1e-5, atol=0.0), (p, fid, got, want)
    assert ed["expected"][(b, 1)] == 2.0 ** 0 + 2.0 ** 1 and ed["expected"][(d, 0)] == 2.0 ** 3
    assert dev.n_contributions == ed["arrivals"] > 300


# ---- metamorphic identities ------------------------------------------------------------------------------------------------------
def _without_mobility(batches):
    out = []
    for b in batches:
        out.append(RawBatch.from_arrays(b.ids, b.peak_off, b.mz, b.intensities, b.precursor_mz, b.precursor_charge, b.isolation_lo,
                                        b.isolation_hi, b.scan_start_time, b.inverse_ion_mobility, b.file_id))
    return out


@pytest.mark.parametrize("combine", [True, False])
def test_no_mobility_anywhere_is_sage_hip_lfq(db, run, combine):
    """(a) the new entry point without a mobility column — no array at all, or arrays that no spectrum is flagged to have —
    returns what sage_hip_lfq returns, every array, bit for bit, whatever `ims` and the tolerance say."""
    st = LfqSettings(combine_charge_states=combine, mobility_pct_tolerance=0.3)
    args = (run["f"], None, run["art"], run["pq"], run["al"])
    rest = (run["carbon"], run["sulfur"], st, (2, 4))
    plain = _without_mobility(run["batches"])
    want = lfq(*args, plain, *rest, debug=True)
    assert len(want.peptide_idx) > 20
    assert_identical(lfq_im(*args, plain, *rest, debug=True), want)
    flagged_off = _without_mobility(run["batches"])
    for b in flagged_off:
        b.mobility, b.has_mobility = np.full(len(b.mz), 7.0, np.float32), np.zeros(b.n, np.uint8)
    assert_identical(lfq_im(*args, flagged_off, *rest, debug=True), want)


@pytest.mark.parametrize("combine", [True, False])
def test_one_mobility_everywhere_is_the_run_without(db, run, combine):
    """(b) every feature with the same finite ims > 0 and every peak at that mobility: every window holds every peak, so the
    result is the run without mobility — at any tolerance, 0 included (the window [ims, ims])."""
    f = run["f"].copy()
    f["ims"] = F32(0.8731)
    args = (None, run["art"], run["pq"], run["al"])
    plain = _without_mobility(run["batches"])
    same = _without_mobility(run["batches"])
    for b in same:
        b.mobility, b.has_mobility = np.full(len(b.mz), F32(0.8731), np.float32), np.ones(b.n, np.uint8)
    for tol in (1.0, 0.0):
        st = LfqSettings(combine_charge_states=combine, mobility_pct_tolerance=tol)
        rest = (run["carbon"], run["sulfur"], st, (2, 4))
        want = lfq(f, *args, plain, *rest, debug=True)
        assert_identical(lfq_im(f, *args, same, *rest, debug=True), want)
    # and the counter-check: at another mobility nothing arrives
    for b in same:
        b.mobility = np.full(len(b.mz), F32(0.95), np.float32)
    assert len(lfq_im(f, *args, same, *rest, debug=True).peptide_idx) == 0


# ---- why it matters ----------------------------------------------------------------------------------------------------------------
def test_isobaric_coeluting_peptides_are_separated(db):
    """Two peptides' features of equal mass and RT and different ims, their MS1 peaks interleaved (same m/z, alternating
    mobility).  Without the column both grids are the sum of both; with it each gets its own — as the restatement says."""
    rng = np.random.default_rng(44)
    a, b = sorted(int(x) for x in rng.permutation(db.n_peptides)[:2])
    f, art, pq = features_table(db, [(a, 1, 1800.0, 0, 0.5, 0.0), (b, 1, 1800.0, 0, 0.5, 0.0)])
    f["ims"] = [0.85, 1.10]
    settings = R.default_settings(spectral_angle=0.0)
    st = LfqSettings(spectral_angle=0.0)
    fmap = RI.build_feature_map(settings, (2, 3), ref_feats(f, art, pq))
    iso_mz = [_mz_for_mass(F32((F32(1800.0) + F32(i) * R.NEUTRON) / F32(2.0))) for i in range(3)]
    assert all(v is not None for v in iso_mz)
    spectra = []
    for t in np.linspace(0.496, 0.504, 41):
        shape = np.exp(-0.5 * ((t - 0.5) / 0.0015) ** 2)
        mz, it, mob = [], [], []
        for i, rel in enumerate((1.0, 0.9, 0.45)):  # a: intensity 1e6, b: 3e5, interleaved peak by peak
            mz += [iso_mz[i], iso_mz[i]]
            it += [1e6 * rel * shape, 3e5 * rel * shape]
            mob += [0.851, 1.098]
        spectra.append(RawSpectrum(np.array(mz, np.float32), np.array(it, np.float32), 0.0, None, None, float(F32(t)), None, 0,
                                   f"t={t}", mobility=np.array(mob, np.float32)))
    batch = [RawBatch(spectra)]
    cc, ss = peptide_compositions(db.seq_off, db.seq)
    al = unit_alignments(1)
    args = (f, None, art, pq, al)
    with_im = lfq_im(*args, batch, cc, ss, st, (2, 3), debug=True)
    without = lfq(*args, _without_mobility(batch), cc, ss, st, (2, 3), debug=True)
    grids = RI.trace(fmap, ref_spectra(batch), [tuple(x) for x in al.tolist()], 1, True, isotopes_of(db))
    ref, passing, _ = R.quantify(settings, (2, 3), None, None, None, 1, None, grids=grids)
    assert_same(with_im, ref, grids, passing, 1)
    assert with_im.peptide_idx.tolist() == [a, b] == without.peptide_idx.tolist() and with_im.has_peak.all() and without.has_peak.all()
    ia, ib = with_im.areas[:, 0]
    oa, ob = without.areas[:, 0]
    assert without.matrix[0].tobytes() == without.matrix[1].tobytes(), "without mobility both grids receive every peak"
    assert with_im.matrix[0].tobytes() != with_im.matrix[1].tobytes()
    assert ia != oa and ib != ob
    # b's peaks are 0.3 x a's: each trace alone is 1 / 1.3 (a) and 0.3 / 1.3 (b) of the summed one
    assert 1.2 < oa / ia < 1.4 and 3.9 < ob / ib < 4.8


# ---- command line end to end ---------------------------------------------------------------------------------------------------
def test_cli_lfq_im_end_to_end(tmp_path, db):
    """mzML files with per-peak mobility arrays in their MS1 spectra and the precursor mobility in their MS2 scans, through
    sage_amd.cli to lfq.tsv; the restatement fed with this run's own features (results.sage.tsv, its ion_mobility column) and
    the MS1 spectra of the Python reader.  The same files without the arrays take the old entry point."""
    fasta = tmp_path / "db.fasta"
    fasta.write_text(synthetic_fasta(60, seed=11))
    files = synthetic_lcms(db, n_files=3, n_peptides=150, ms1_per_file=300, seed=6, ms1_noise=40, ms2_per_peptide=2)
    _, mobility = synthetic_ion_mobility(db, files, seed=9)
    for j in range(0, len(mobility[2]), 4):  # spectra with and without the array in one file
        mobility[2][j] = None
    paths = write_lcms(str(tmp_path / "mzml"), files, mobility=mobility)
    plain_paths = write_lcms(str(tmp_path / "mzml_plain"), files)
    base = {"database": {"fasta": str(fasta), "enzyme": {"missed_cleavages": 1, "cleave_at": "KR", "restrict": "P"},
                         "static_mods": {"C": 57.0215}},
            "precursor_tol": {"ppm": [-10, 10]}, "fragment_tol": {"ppm": [-10, 10]}, "min_peaks": 10, "min_matched_peaks": 4}
    quant = {"lfq": True, "lfq_settings": {"peptide_q_value": 1.0, "mobility_pct_tolerance": 1.0}}
    outs = {}
    for name, extra in (("im", {"mzml_paths": paths, "quant": quant}), ("plain", {"mzml_paths": plain_paths, "quant": quant})):
        cfg = tmp_path / f"{name}.json"
        cfg.write_text(json.dumps(dict(base, **extra)))
        outs[name] = tmp_path / name
        subprocess.run([sys.executable, "-m", "sage_amd.cli", str(cfg), "-o", str(outs[name])], cwd=ROOT, check=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    summary = json.load(open(outs["im"] / "results.json"))["summary"]
    assert summary["lfq_ion_mobility"] is True
    assert json.load(open(outs["plain"] / "results.json"))["summary"]["lfq_ion_mobility"] is False
    lines = (outs["im"] / "results.sage.tsv").read_text().splitlines()
    col = {k: i for i, k in enumerate(lines[0].split("\t"))}
    rows = [l.split("\t") for l in lines[1:]]
    idx_of = {db.peptide_string(i): i for i in range(db.n_peptides)}
    names = [os.path.basename(p) for p in paths]
    feats = dict(peptide_idx=np.array([idx_of[r[col["peptide"]]] for r in rows]), label=np.array([int(r[col["label"]]) for r in rows]),
                 calcmass=np.array([F32(r[col["calcmass"]]) for r in rows]),
                 file_id=np.array([names.index(r[col["filename"]]) for r in rows]),
                 aligned_rt=np.array([F32(r[col["aligned_rt"]]) for r in rows]), peptide_q=np.array([F32(r[col["peptide_q"]]) for r in rows]),
                 ims=np.array([F32(r[col["ion_mobility"]]) for r in rows]))
    assert (feats["ims"] > 0.5).mean() > 0.9, "the search carries the MS2 scans' mobility into Feature.ims"
    from sage_amd import output
    from sage_amd.mzml import read_mzml
    spectra = []
    for fid, p in enumerate(paths):
        for s in read_mzml(p, fid, 1):
            if s.mobility is None:
                (m, it), mob = R.process_ms1(s.mz, s.intensity), None
            else:
                m, it, mob = RI.process_ms1(s.mz, s.intensity, s.mobility)
            spectra.append((fid, F32(s.scan_start_time), m, it, mob))
    assert 0 < sum(s[4] is None for s in spectra) < len(spectra)
    settings = R.default_settings(peptide_q_value=1.0, mobility_pct_tolerance=1.0)
    alignments = [(a["file_id"], F32(a["max_rt"]), F32(a["slope"]), F32(a["intercept"])) for a in summary["alignments"]]
    ref, passing, _ = RI.quantify(settings, (2, 4), feats, spectra, alignments, 3, isotopes_of(db))
    got = (outs["im"] / "lfq.tsv").read_text().splitlines()
    assert got[0].split("\t") == output.LFQ_HEADERS + names
    want = [k for k in sorted(ref) if not k[2] and ref[k]["peak"]]
    assert len(want) >= 20 and len(got) - 1 == len(want)
    for line, k in zip(got[1:], want):
        r = ref[k]
        v = line.split("\t")
        assert v[0] == db.peptide_string(k[0]) and v[1] == "-1" and v[2] == db.peptide_proteins(k[0])
        assert v[3] == output.ryu_f32(r["q_value"]) and v[6:] == [output.ryu_f64(a) for a in r["areas"]]
        assert ulp_close(float(v[4]), r["score"]) and ulp_close(float(v[5]), r["spectral_angle"])
    assert summary["q_precursor"] == passing
    # the mobility windows changed the areas: the run over the same spectra without the arrays differs
    assert (outs["plain"] / "lfq.tsv").read_text().splitlines()[1:] != got[1:]
    assert (outs["plain"] / "results.sage.tsv").read_text().count("\n") == len(lines)
