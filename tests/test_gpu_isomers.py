"""Positional isomers of reported PSMs scored on the device (sage_hip_score_candidates_resident): equal to the
oracle where the oracle has an answer (the candidates a search reports), equal to the second reading of scoring.rs
(tests/second_reading.py through tests/isomers_reference.py) everywhere else — candidates no search reports, the split b / y
fields, the spectrum after a chimera's peak removal —, the launch shapes that can go wrong, invalid input, planted modification
sites, and the CLI's isomers.sage.tsv."""
import json
import os

import numpy as np
import pytest

import isomers_reference as IR
import oracle_lib
import second_reading as SR
from sage_amd import _lib as L
from sage_amd import cli, output
from sage_amd.api import (DatabaseParameters, DeviceDatabase, ProcessedSpectrum, RawBatch, RawSpectrum, Scorer, ScorerParams,
                          SpectrumBatch, SpectrumProcessor, Tolerance)
from sage_amd.mzml import read_mzml, write_mzml
from sage_amd.synthetic import synthetic_fasta, synthetic_spectra

pytestmark = pytest.mark.gpu

PROTON = 1.0072764
WIDE = Tolerance("ppm", -100.0, 100.0)  # with every charge tried: candidates of two or three charges in one spectrum's list
FASTA = (60, 7)  # the world the feature was planned on: 73 708 peptides, groups of up to 120 placements


class World:
    """A host database, its device copy, its isomer groups and (made on first use) its oracle copy"""

    def __init__(self, dbkw, fasta=FASTA):
        self.dbp = DatabaseParameters(**dbkw)
        self.host = self.dbp.build(synthetic_fasta(*fasta))
        self.dev = DeviceDatabase(self.host, 0)
        self.groups = self.host.isomer_groups()
        self._orc = None

    @property
    def orc(self):
        if self._orc is None:
            self._orc = oracle_lib.OracleDb.from_product(self.host)
        return self._orc

    def spectra(self, n, seed, **kw):
        sp = SpectrumProcessor(150, True, 0.0)
        kw = dict(dict(varmod_frac=0.8, varmod_residues="STYM"), **kw)
        return SpectrumBatch.from_spectra([sp.process(r) for r in synthetic_spectra(self.host, n, seed, **kw)])


class Search:
    """One scorer, one resident batch and the PSMs the device reported for it"""

    def __init__(self, world, params, batch=None, dbatch=None, scorer=None):
        self.world, self.params = world, params
        self.scorer = scorer or Scorer(world.dev, params)
        self.dbatch = dbatch if dbatch is not None else self.scorer.upload(batch)
        feats, counts = self.scorer.score_resident(self.dbatch)
        self.feats, self.counts = feats.copy(), counts.copy()
        self.report = params.report_psms

    def candidates(self, lists, charges=None):
        """lists: {slot: [peptide, ...]}, charges: {slot: [charge, ...]} or None -> {slot: structured array}"""
        n_slots = self.dbatch.n * self.report
        lens = np.zeros(n_slots, dtype=np.int64)
        for s, v in lists.items():
            lens[s] = len(v)
        off = np.zeros(n_slots + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        order = sorted(lists)
        pep = np.array([p for s in order for p in lists[s]], dtype=np.uint32)
        z = None if charges is None else np.array([c for s in order for c in charges[s]], dtype=np.uint8)
        out = self.scorer.score_candidates(self.dbatch, self.feats, self.counts, off, pep, z)
        assert len(out) == len(pep) and not out["pad"].any()
        return {s: out[int(off[s]):int(off[s + 1])] for s in order}


@pytest.fixture(scope="module")
def world(gpu_required):
    return World(IR.PHOSPHO_DB)


@pytest.fixture(scope="module")
def aby_world(gpu_required):
    return World(dict(IR.PHOSPHO_DB, ion_kinds=["a", "b", "y"]), fasta=(40, 21))


# ---- equal to the oracle where the oracle has an answer --------------------------------------------------------------------
def _hold_to_the_oracle(w, params, batch, context):
    se = Search(w, params, batch)
    of, oc, _, _ = w.orc.score(params, batch)
    assert np.array_equal(se.counts, oc), context
    lists, charges = {}, {}
    for i in range(batch.n):
        if oc[i]:
            lists[i * se.report] = [int(of[i, r]["peptide_idx"]) for r in range(int(oc[i]))]
            charges[i * se.report] = [int(of[i, r]["charge"]) for r in range(int(oc[i]))]
    got = se.candidates(lists, charges)
    n, seen_charges, mixed = 0, set(), 0
    for i in range(batch.n):
        mixed += len(set(charges.get(i * se.report, []))) > 1
        for r in range(int(oc[i])):
            g, o, ctx = got[i * se.report][r], of[i, r], f"{context} spectrum {i} oracle rank {r + 1}"
            assert int(g["matched_b"]) + int(g["matched_y"]) == int(o["matched_peaks"]), ctx
            assert int(g["longest_b"]) == int(o["longest_b"]) and int(g["longest_y"]) == int(o["longest_y"]), ctx
            assert np.float32(g["average_ppm"]).view(np.uint32) == np.float32(o["average_ppm"]).view(np.uint32), ctx
            assert (np.float32(g["summed_b"]) + np.float32(g["summed_y"])).view(np.uint32) == np.float32(o["ms2_intensity"]).view(np.uint32), ctx
            # (both score types: the f64 ln and the f32 ln_1p are correctly rounded on both sides)
            assert np.float64(g["hyperscore"]).view(np.uint64) == np.float64(o["hyperscore"]).view(np.uint64), \
                f"{ctx}: hyperscore {g['hyperscore']!r} vs {o['hyperscore']!r}"
            seen_charges.add(int(o["charge"]))
            n += 1
    return n, seen_charges, mixed


@pytest.mark.parametrize("score_type", ["SageHyperScore", "OpenMSHyperScore"])
def test_reported_candidates_equal_the_oracle(world, score_type):
    params = ScorerParams(report_psms=20, override_precursor_charge=True, min_matched_peaks=2, precursor_tol=WIDE, score_type=score_type)
    n, zs, mixed = _hold_to_the_oracle(world, params, world.spectra(220, 31), score_type)
    assert n > 500 and zs == {2, 3, 4} and mixed > 10  # charges 2-4 mix inside one spectrum's list


def test_reported_candidates_equal_the_oracle_three_ion_kinds(aby_world):
    params = ScorerParams(report_psms=20, override_precursor_charge=True, min_matched_peaks=2, precursor_tol=WIDE)
    n, zs, mixed = _hold_to_the_oracle(aby_world, params, aby_world.spectra(200, 32), "a, b, y")
    assert n > 500 and zs == {2, 3, 4} and mixed > 10


# ---- equal to the second reading everywhere else ---------------------------------------------------------------------------
def _psm_states(sr, batch, se, i):
    s = SR.spectrum_of(batch, i)
    psms = [(int(se.feats[i, r]["peptide_idx"]), int(se.feats[i, r]["charge"])) for r in range(int(se.counts[i]))]
    return IR.states(sr, s["masses"], s["intensities"], psms)


def test_isomers_and_unreported_candidates_equal_the_second_reading(world):
    params = ScorerParams(report_psms=2)
    batch = world.spectra(200, 33)
    se = Search(world, params, batch)
    sr = IR.second_scorer(world.host, world.dbp, params)
    rng = np.random.default_rng(8)
    lists = {}
    for i in range(batch.n):
        for r in range(int(se.counts[i])):
            pep = int(se.feats[i, r]["peptide_idx"])
            # every isomer, and two peptides of nearly the same mass that share nothing with the spectrum but chance
            near = [int(p) for p in np.clip(pep + rng.integers(-40, 40, 2), 0, world.host.n_peptides - 1)]
            lists[i * 2 + r] = IR.others(world.groups, pep) + near
    got = se.candidates(lists)
    n_iso = n_zero = n_below = 0
    for slot, peps in lists.items():
        i, r = divmod(slot, 2)
        s = SR.spectrum_of(batch, i)
        for j, pep in enumerate(peps):
            want = IR.score(sr, s["masses"], s["intensities"], pep, int(se.feats[i, r]["charge"]))
            IR.assert_score_equal(got[slot][j], want, 1e-12, f"spectrum {i} rank {r + 1} candidate {pep}")
            m = want["matched_b"] + want["matched_y"]
            n_iso += j < len(peps) - 2
            n_zero += m == 0
            n_below += 0 < m < params.min_matched_peaks
            if m == 0:
                assert np.isnan(got[slot][j]["average_ppm"]) and got[slot][j]["hyperscore"] == 2.0  # ln(1) + lnfact(0) * 2
    assert n_iso > 500 and n_zero > 50 and n_below > 20, (n_iso, n_zero, n_below)


def test_chimera_ranks_see_the_spectrum_after_peak_removal(world):
    params = ScorerParams(chimera=True, report_psms=3, min_matched_peaks=1)
    batch = world.spectra(200, 34, chimeric=2)
    se = Search(world, params, batch)
    sr = IR.second_scorer(world.host, world.dbp, params)
    lists = {}
    for i in range(batch.n):
        for r in range(int(se.counts[i])):
            pep = int(se.feats[i, r]["peptide_idx"])
            lists[i * 3 + r] = [pep] + IR.others(world.groups, pep)
    got = se.candidates(lists)
    n_later = n_changed = 0
    for i in range(batch.n):
        states = _psm_states(sr, batch, se, i)
        for r in range(int(se.counts[i])):
            f, own, ctx = se.feats[i, r], got[i * 3 + r][0], f"spectrum {i} rank {r + 1}"
            # slot r's own peptide reproduces PSM r: the peak removal of the ranks before it was replayed
            assert int(own["matched_b"]) + int(own["matched_y"]) == int(f["matched_peaks"]), ctx
            assert (int(own["longest_b"]), int(own["longest_y"])) == (int(f["longest_b"]), int(f["longest_y"])), ctx
            assert np.float32(own["average_ppm"]).view(np.uint32) == np.float32(f["average_ppm"]).view(np.uint32), ctx
            assert (np.float32(own["summed_b"]) + np.float32(own["summed_y"])).view(np.uint32) == np.float32(f["ms2_intensity"]).view(np.uint32), ctx
            assert np.float64(own["hyperscore"]).view(np.uint64) == np.float64(f["hyperscore"]).view(np.uint64), ctx
            masses, intens = states[r]
            for j, pep in enumerate(lists[i * 3 + r]):
                IR.assert_score_equal(got[i * 3 + r][j], IR.score(sr, masses, intens, pep, int(f["charge"])), 1e-12, f"{ctx} candidate {pep}")
            n_later += r > 0
            n_changed += r > 0 and len(masses) < len(states[0][0])
    assert n_later > 50 and n_changed == n_later, (n_later, n_changed)


# ---- shapes that can go wrong ----------------------------------------------------------------------------------------------
def _planted(sr, pep, z_frag, keep=None, base=1000.0):
    """(masses, intensities) made of the ions of `pep` at fragment charges 1 .. z_frag (`keep`: a mask over them), ascending"""
    ions = np.concatenate([sr.db.ion_series(pep, k) for k in sr.kinds])
    m = np.concatenate([ions / np.float32(z) for z in range(1, z_frag + 1)]).astype(np.float32)
    if keep is not None:
        m = m[keep(len(m))]
    m = np.unique(m)
    return m, (np.float32(base) + np.float32(7.0) * np.arange(len(m), dtype=np.float32) % np.float32(97.0)).astype(np.float32)


def _spectrum(masses, intensities, mono, z, k):
    return ProcessedSpectrum(masses, intensities, float(np.sum(intensities, dtype=np.float32)), float(np.float32((float(mono) + z * PROTON) / z)),
                             z, None, 0.01 * k, None, 0, f"scan={k + 1}")


def _peptide_of_length(host, length, skip=0):
    lens = np.diff(host.seq_off.astype(np.int64))
    return int(np.flatnonzero((lens == length) & (host.decoy == 0))[skip])


def test_trip_boundaries_of_64_65_and_129_items(gpu_required):
    """One ion kind, so that a candidate's (ion, fragment charge) items can fill exactly 64 (32 ions x 2 charges), 65 (13 x 5)
    and 2 x 64 + 1 (43 x 3) lanes; the spectra hold the candidates' own fragments at every charge, three in four of them, so the
    matches fall on both sides of every trip boundary."""
    w = World(dict(IR.PHOSPHO_DB, ion_kinds=["y"]), fasta=(40, 21))
    params = ScorerParams(report_psms=1, min_matched_peaks=1)
    sr = IR.second_scorer(w.host, w.dbp, params)
    shapes = [(33, 3, 64), (14, 6, 65), (44, 4, 129)]  # peptide length, precursor charge -> items
    peps = [_peptide_of_length(w.host, n) for n, _, _ in shapes]
    rng = np.random.default_rng(3)
    spectra = []
    for k, (pep, (n, z, items)) in enumerate(zip(peps, shapes)):
        assert (n - 1) * (SR.max_fragment_charge(None, z) - 1) == items
        m, it = _planted(sr, pep, z - 1, keep=lambda size: rng.random(size) < 0.75)
        spectra.append(_spectrum(m, it, w.host.pep_mono[pep], min(z, 4), k))
    batch = SpectrumBatch.from_spectra(spectra)
    se = Search(w, params, batch)
    assert np.all(se.counts == 1)
    # every candidate on every spectrum, at its own charge
    lists = {i: peps for i in range(3)}
    charges = {i: [z for _, z, _ in shapes] for i in range(3)}
    got = se.candidates(lists, charges)
    for i in range(3):
        s = SR.spectrum_of(batch, i)
        for j, pep in enumerate(peps):
            want = IR.score(sr, s["masses"], s["intensities"], pep, shapes[j][1])
            IR.assert_score_equal(got[i][j], want, 1e-12, f"spectrum {i} candidate {j}")
            if i == j:  # its own spectrum: matches in the first and in the last trip
                assert want["matched_y"] > 0.6 * shapes[j][2] and want["matched_b"] == 0


def _crafted_batch(w, sr):
    """Processed spectra made by hand: [0] a member of a two-placement group, [1] noise (no PSM), [2] a member of the largest
    group, [3] one peak, [4] 37 peaks, [5] a precursor of charge 2 and [6] of charge 4 for one peptide"""
    group_of, group_off, members = w.groups
    sizes = np.diff(group_off.astype(np.int64))
    lens = np.diff(w.host.seq_off.astype(np.int64))
    first = members[group_off[:-1].astype(np.int64)]
    ok = (w.host.decoy[first] == 0) & (lens[first] >= 12)
    pair = int(first[np.flatnonzero((sizes == 2) & ok)[0]])
    large = int(first[np.flatnonzero(sizes == sizes.max())[0]])
    assert sizes.max() > 64 and w.host.decoy[large] == 0
    some = int(first[np.flatnonzero((sizes >= 3) & ok & (lens[first] >= 20))[0]])
    rng = np.random.default_rng(4)
    noise = np.sort(rng.uniform(200.0, 1500.0, 60).astype(np.float32))
    m1, i1 = _planted(sr, some, 1)
    m37, i37 = _planted(sr, some, 1, keep=lambda size: np.arange(size) < 37)
    specs = [_spectrum(*_planted(sr, pair, 1), w.host.pep_mono[pair], 2, 0),
             _spectrum(noise, rng.lognormal(6.0, 1.0, 60).astype(np.float32), 2.0 * 4000.0, 2, 1),  # (no peptide weighs 8000)
             _spectrum(*_planted(sr, large, 1), w.host.pep_mono[large], 2, 2),
             _spectrum(m1[len(m1) // 2:len(m1) // 2 + 1], i1[:1], w.host.pep_mono[some], 2, 3),
             _spectrum(m37, i37, w.host.pep_mono[some], 3, 4),
             _spectrum(*_planted(sr, some, 3), w.host.pep_mono[some], 2, 5),
             _spectrum(*_planted(sr, some, 3), w.host.pep_mono[some], 4, 6)]
    assert len(m37) == 37
    return SpectrumBatch.from_spectra(specs), pair, large, some


def test_group_sizes_peak_counts_and_charges(world):
    params = ScorerParams(report_psms=3, min_matched_peaks=1)
    sr = IR.second_scorer(world.host, world.dbp, params)
    batch, pair, large, some = _crafted_batch(world, sr)
    se = Search(world, params, batch)
    # a spectrum without a PSM between two that have some; fewer PSMs than report_psms; one peak; a peak count off the powers of two
    assert se.counts[0] >= 1 and se.counts[1] == 0 and se.counts[2] >= 1 and se.counts[3] >= 1
    assert np.any((se.counts > 0) & (se.counts < 3))
    assert [int(batch.peak_off[k + 1] - batch.peak_off[k]) for k in (3, 4)] == [1, 37]
    lists = {}
    for i in range(batch.n):
        for r in range(int(se.counts[i])):
            lists[i * 3 + r] = IR.others(world.groups, int(se.feats[i, r]["peptide_idx"]))
    lists = {s: v for s, v in lists.items() if v}
    sizes = {s: len(v) for s, v in lists.items()}
    assert 1 in sizes.values() and max(sizes.values()) > 64, sizes  # one isomer; more than a wavefront of them
    assert int(world.groups[0][int(se.feats[0, 0]["peptide_idx"])]) == int(world.groups[0][pair])
    assert int(world.groups[0][int(se.feats[2, 0]["peptide_idx"])]) == int(world.groups[0][large])
    assert {int(se.feats[5, 0]["charge"]), int(se.feats[6, 0]["charge"])} == {2, 4}  # one fragment charge; three
    got = se.candidates(lists)
    for slot, peps in lists.items():
        i, r = divmod(slot, 3)
        s = SR.spectrum_of(batch, i)
        for j, pep in enumerate(peps):
            IR.assert_score_equal(got[slot][j], IR.score(sr, s["masses"], s["intensities"], pep, int(se.feats[i, r]["charge"])), 1e-12,
                                  f"spectrum {i} rank {r + 1} candidate {pep}")
    # no candidate at all: nothing to score, nothing launched
    empty = se.scorer.score_candidates(se.dbatch, se.feats, se.counts, np.zeros(batch.n * 3 + 1, np.uint64), np.zeros(0, np.uint32))
    assert len(empty) == 0 and se.scorer.last_candidates_timing() == (0.0, 0.0)


def test_a_spectrum_beyond_64_kb_of_lds(world):
    """7 000 peaks are 70 000 bytes of dynamic LDS: more than a launch gets unless the kernel's limit was raised"""
    params = ScorerParams(report_psms=1)
    sr = IR.second_scorer(world.host, world.dbp, params)
    _, group_off, members = world.groups
    sizes = np.diff(group_off.astype(np.int64))
    lens = np.diff(world.host.seq_off.astype(np.int64))
    first = members[group_off[:-1].astype(np.int64)]
    pep = int(first[np.flatnonzero((sizes >= 3) & (world.host.decoy[first] == 0) & (lens[first] >= 20))[0]])
    m, it = _planted(sr, pep, 1, base=50000.0)
    rng = np.random.default_rng(6)
    noise = np.setdiff1d(np.unique(rng.uniform(150.0, 3000.0, 7200).astype(np.float32)), m)[:7000 - len(m)]
    masses = np.concatenate([m, noise])
    intens = np.concatenate([it, rng.lognormal(5.0, 1.0, len(noise)).astype(np.float32)])
    order = np.argsort(masses, kind="stable")
    batch = SpectrumBatch.from_spectra([_spectrum(masses[order], intens[order], world.host.pep_mono[pep], 2, 0)])
    assert int(batch.peak_off[1]) == 7000 and 7000 * 10 > 64 * 1024
    se = Search(world, params, batch)
    assert se.counts[0] == 1
    lists = {0: IR.others(world.groups, int(se.feats[0, 0]["peptide_idx"]))}
    assert len(lists[0]) >= 2
    got = se.candidates(lists)
    for j, cand in enumerate(lists[0]):
        IR.assert_score_equal(got[0][j], IR.score(sr, batch.masses, batch.intensities, cand, 2), 1e-12, f"candidate {cand}")


def test_a_spectrum_that_preprocessing_left_without_peaks(world):
    """process_upload keeps a spectrum below min_peaks in the batch with zero peaks: it has no PSM and no candidates, and its
    neighbours are scored on their own peaks"""
    params = ScorerParams(report_psms=1)
    raws = synthetic_spectra(world.host, 6, 35, varmod_frac=0.9, varmod_residues="STYM", pure_noise_frac=0.0)
    short = raws[2]
    raws[2] = RawSpectrum(short.mz[:9], short.intensity[:9], short.precursor_mz, short.precursor_charge, None, 0.02, None, 0, "short")
    scorer = Scorer(world.dev, params)
    dbatch, kept = scorer.process_upload(RawBatch(raws), 150, True, 0.0, 15)
    se = Search(world, params, dbatch=dbatch, scorer=scorer)
    off, masses, intens, _ = dbatch.download()
    assert kept[2] <= 9 and off[3] == off[2] and se.counts[2] == 0
    sr = IR.second_scorer(world.host, world.dbp, params)
    lists = {i: IR.others(world.groups, int(se.feats[i, 0]["peptide_idx"])) for i in range(6) if se.counts[i]}
    lists = {s: v for s, v in lists.items() if v}
    assert min(lists) < 2 < max(lists)
    got = se.candidates(lists)
    for i, peps in lists.items():
        m, it = masses[int(off[i]):int(off[i + 1])], intens[int(off[i]):int(off[i + 1])]
        for j, pep in enumerate(peps):
            IR.assert_score_equal(got[i][j], IR.score(sr, m, it, pep, int(se.feats[i, 0]["charge"])), 1e-12, f"spectrum {i} candidate {pep}")


# ---- invalid input -----------------------------------------------------------------------------------------------------------
def test_invalid_input_is_refused_before_any_launch(world):
    params = ScorerParams(report_psms=2)
    batch = world.spectra(40, 36)
    se = Search(world, params, batch)
    with_psm = int(np.flatnonzero(se.counts == 1)[0])  # one PSM: slot 1 of the spectrum holds none
    pep = int(se.feats[with_psm, 0]["peptide_idx"])
    n_slots = batch.n * 2

    def call(off, peps, charges=None):
        return se.scorer.score_candidates(se.dbatch, se.feats, se.counts, np.asarray(off, np.uint64), np.asarray(peps, np.uint32), charges)

    good = np.zeros(n_slots + 1, np.uint64)
    good[with_psm * 2 + 1:] = 2
    before = call(good, [pep, pep])
    decreasing = good.copy()
    decreasing[with_psm * 2 + 1] = 2
    decreasing[with_psm * 2 + 2] = 1
    beyond = np.zeros(n_slots + 1, np.uint64)
    beyond[with_psm * 2 + 2:] = 1  # a list on slot 1, beyond counts[i] == 1
    for name, args in [("decreasing cand_off", (decreasing, [pep, pep])), ("slot beyond counts", (beyond, [pep])),
                       ("peptide index n_peptides", (good, [pep, world.host.n_peptides])),
                       ("charge 255", (good, [pep, pep], [2, 255]))]:
        with pytest.raises(L.SageHipError, match="status 1") as err:
            call(*args)
        assert "sage_hip_score_candidates_resident" in str(err.value), name
    # the batch scores normally afterwards
    after = call(good, [pep, pep])
    assert before.tobytes() == after.tobytes() and before[0].tobytes() == before[1].tobytes()
    feats, counts = se.scorer.score_resident(se.dbatch)
    assert np.array_equal(counts, se.counts) and feats[with_psm, 0].tobytes() == se.feats[with_psm, 0].tobytes()


# ---- planted sites ---------------------------------------------------------------------------------------------------------
def _delta_and_best(se, lists, got, slot):
    f = se.feats.reshape(-1)[slot]
    hyper = [float(x) for x in got[slot]["hyperscore"]]
    best, j = IR.pick_best(lists[slot], hyper)
    return float(f["hyperscore"]) - hyper[j], best


def test_planted_sites(world):
    """Spectra made of ALL fragments of one placement: the search reports it and every other placement scores lower.  Spectra made
    of the fragments two placements share: the two tie, and the tie goes to the lower index.  The restatement says so first."""
    params = ScorerParams(report_psms=1)
    sr = IR.second_scorer(world.host, world.dbp, params)
    group_of, group_off, members = world.groups
    lens = np.diff(world.host.seq_off.astype(np.int64))
    sizes = np.diff(group_off.astype(np.int64))
    specs, plan, n_kind = [], [], {"one": 0, "two": 0}
    for g in np.flatnonzero((sizes >= 3) & (sizes <= 12)):
        if min(n_kind.values()) >= 4:
            break
        mem = [int(p) for p in members[int(group_off[g]):int(group_off[g + 1])]]
        if world.host.decoy[mem[0]] or not 12 <= lens[mem[0]] <= 30:
            continue
        chosen = mem[len(mem) // 2]
        m, it = _planted(sr, chosen, 1)
        hyper = {p: IR.score(sr, m, it, p, 2)["hyperscore"] for p in mem}
        if n_kind["one"] < 4 and all(hyper[chosen] > hyper[p] for p in mem if p != chosen):
            specs.append(_spectrum(m, it, world.host.pep_mono[chosen], 2, len(specs)))
            plan.append(("one", chosen, mem, hyper))
            n_kind["one"] += 1
            continue
        a, b = mem[0], mem[1]
        ions = [np.concatenate([sr.db.ion_series(p, k) for k in sr.kinds]) for p in (a, b)]
        shared = np.unique(ions[0][ions[0].view(np.uint32) == ions[1].view(np.uint32)])
        if len(shared) < 8 or n_kind["two"] >= 4:
            continue
        it = (np.float32(500.0) + np.arange(len(shared), dtype=np.float32)).astype(np.float32)
        hyper = {p: IR.score(sr, shared, it, p, 2)["hyperscore"] for p in mem}
        if hyper[a] == hyper[b] == max(hyper.values()):
            specs.append(_spectrum(shared, it, world.host.pep_mono[a], 2, len(specs)))
            plan.append(("two", a, mem, hyper))
            n_kind["two"] += 1
    assert n_kind["one"] >= 3 and n_kind["two"] >= 3, n_kind
    batch = SpectrumBatch.from_spectra(specs)
    se = Search(world, params, batch)
    assert np.all(se.counts == 1)
    lists = {i: IR.others(world.groups, int(se.feats[i, 0]["peptide_idx"])) for i in range(batch.n)}
    got = se.candidates(lists)
    for i, (kind, pep, mem, hyper) in enumerate(plan):
        reported = int(se.feats[i, 0]["peptide_idx"])
        delta, best = _delta_and_best(se, lists, got, i)
        if kind == "one":
            assert reported == pep and delta > 0.0, (i, reported, pep, delta)
        else:
            top = [p for p in mem if hyper[p] == max(hyper.values())]
            assert reported in top and delta == 0.0 and best == min(p for p in top if p != reported), (i, reported, top, delta, best)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def _read_tsv(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:-1]]


def _restated_rows(host, dbp, cfg, files, result_rows, hdr):
    """isomers.sage.tsv from the restatement: the file's spectra processed on the host, searched through the API for the PSMs
    (psm_id counts them in (file, spectrum, rank) order from 1), every other placement scored by the second reading"""
    search = cli.search_parameters(cfg)
    params = cli.scorer_params(search)
    sr = IR.second_scorer(host, dbp, params)
    groups = IR.isomer_groups(host)
    scorer = Scorer(DeviceDatabase(host, 0), params)
    sp = SpectrumProcessor(search["max_peaks"], search["deisotope"], 0.0)
    by_id, psm_id = {}, 1
    for k, path in enumerate(files):
        proc = [q for q in (sp.process(r) for r in read_mzml(path, k)) if len(q.masses) >= search["min_peaks"]]
        batch = SpectrumBatch.from_spectra(proc)
        feats, counts = scorer.score(batch)
        for i in range(batch.n):
            s = SR.spectrum_of(batch, i)
            for r in range(int(counts[i])):
                f = feats[i, r]
                peps = IR.others(groups, int(f["peptide_idx"]))
                if peps:
                    sc = [IR.score(sr, s["masses"], s["intensities"], p, int(f["charge"])) for p in peps]
                    best, j = IR.pick_best(peps, [x["hyperscore"] for x in sc])
                    by_id[psm_id] = (host.peptide_string(int(f["peptide_idx"])), len(peps), host.peptide_string(best), sc[j]["hyperscore"],
                                     sc[j]["matched_b"] + sc[j]["matched_y"], float(f["hyperscore"]) - sc[j]["hyperscore"],
                                     float(f["hyperscore"]))
                psm_id += 1
    return [(int(r[hdr.index("psm_id")]),) + by_id[int(r[hdr.index("psm_id")])] for r in result_rows if int(r[hdr.index("psm_id")]) in by_id]


def _assert_isomer_file(path, want):
    hdr, rows = _read_tsv(path)
    assert hdr == output.ISOMER_HEADERS
    assert len(rows) == len(want)
    for r, w in zip(rows, want):
        assert (int(r[0]), r[1], int(r[2]), r[3], int(r[5])) == (w[0], w[1], w[2], w[3], w[5]), (r, w)
        # f64, as tests/test_scoring_second_reading.py compares it: 1e-12 relative to the hyperscores
        scale = max(abs(w[4]), abs(w[7]), 1.0)
        assert abs(float(r[4]) - w[4]) <= 1e-12 * scale and abs(float(r[6]) - w[6]) <= 2e-12 * scale, (r, w)
        assert r[4] == output.ryu_f64(float(r[4])) and r[6] == output.ryu_f64(float(r[6]))


@pytest.mark.parametrize("flow", ["plain", "devices_0_0", "prefilter"])
def test_cli_writes_isomers_and_changes_nothing_else(tmp_path, gpu_required, flow):
    fasta = synthetic_fasta(40, 21)
    fa = str(tmp_path / "db.fasta")
    open(fa, "w").write(fasta)
    dbj = dict(IR.PHOSPHO_DB, fasta=fa)
    if flow == "prefilter":
        dbj.update(prefilter=True, prefilter_chunk_size=16)
    dbp = DatabaseParameters.from_json(dbj)
    full = DatabaseParameters.from_json(dict(dbj, prefilter=False)).build(fasta)
    files = []
    for k in range(2):
        files.append(str(tmp_path / f"run{k}.mzML"))
        write_mzml(files[-1], synthetic_spectra(full, 110, seed=70 + k, varmod_frac=0.8, varmod_residues="STYM"))
    cfg = {"database": dbj, "precursor_tol": {"ppm": [-10, 10]}, "fragment_tol": {"ppm": [-10, 10]}, "report_psms": 2,
           "annotate_matches": True, "mzml_paths": files}
    kw = dict(devices=[0, 0]) if flow == "devices_0_0" else {}
    plain, iso = str(tmp_path / "plain"), str(tmp_path / "iso")
    s0 = cli.run(cfg, files, plain, log=lambda m: None, write_pin=True, **kw)
    s1 = cli.run(dict(cfg, score_isomers=True), files, iso, log=lambda m: None, write_pin=True, **kw)
    # without the key: no file, no new summary keys; with it: one more path, every other file byte for byte the same
    assert not os.path.exists(os.path.join(plain, "isomers.sage.tsv"))
    assert "isomer_rows" not in s0 and "isomer_ms" not in s0 and set(s1) - set(s0) == {"isomer_rows", "isomer_ms"}
    ip = os.path.join(iso, "isomers.sage.tsv")
    assert s1["output_paths"] == [p.replace(plain, iso) for p in s0["output_paths"][:2]] + [ip] + \
        [p.replace(plain, iso) for p in s0["output_paths"][2:]]
    assert json.load(open(os.path.join(iso, "results.json")))["output_paths"] == s1["output_paths"]
    for name in ("results.sage.tsv", "matched_fragments.sage.tsv", "results.sage.pin"):
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(iso, name), "rb").read(), name
    host = full
    if flow == "prefilter":  # the database the search ran on: the peptides the first pass kept
        sp = cli.search_parameters(cfg)
        host = cli.prefilter_peptides(dbp, fasta, 16, dbp.num_targets(fasta), sp, files, SpectrumProcessor(150, True, 0.0), 0, False,
                                      lambda m: None)
        assert 0 < host.n_peptides < full.n_peptides
    hdr, rows = _read_tsv(os.path.join(iso, "results.sage.tsv"))
    want = _restated_rows(host, dbp, cfg, files, rows, hdr)
    assert s1["isomer_rows"] == len(want) > 20
    _assert_isomer_file(ip, want)
