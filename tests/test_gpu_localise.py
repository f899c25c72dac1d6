"""Site localisation of reported PSMs on the device (sage_hip_localise_resident) against the plain restatement of
tests/localise_reference.py, in the worlds of tests/test_gpu_isomers.py: every integer (the depth counts of every candidate, the
best and the second placement, the site-determining items and their counts, the depth) for equality, the three f64 values to
1e-12; the launch shapes that can go wrong, refused input, and the CLI's localisation.sage.tsv."""
import json
import math
import os

import numpy as np
import pytest

import isomers_reference as IR
import localise_reference as LR
import second_reading as SR
from sage_amd import _lib as L
from sage_amd import cli, output
from sage_amd.api import (DatabaseParameters, DeviceDatabase, RawBatch, RawSpectrum, Scorer, ScorerParams, SpectrumBatch,
                          SpectrumProcessor)
from sage_amd.mzml import read_mzml, write_mzml
from sage_amd.synthetic import synthetic_fasta, synthetic_spectra
from test_gpu_isomers import Search, World, _crafted_batch, _planted, _psm_states, _read_tsv, _spectrum

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(gpu_required):
    return World(IR.PHOSPHO_DB)


def _localise(se, lists, charges=None, per_candidate=True):
    """lists: {slot: [peptide, ...]} -> (slot records, {slot: depth counts} | None)"""
    n_slots = se.dbatch.n * se.report
    lens = np.zeros(n_slots, dtype=np.int64)
    for s, v in lists.items():
        lens[s] = len(v)
    off = np.zeros(n_slots + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    order = sorted(lists)
    pep = np.array([p for s in order for p in lists[s]], dtype=np.uint32)
    z = None if charges is None else np.array([c for s in order for c in charges[s]], dtype=np.uint8)
    got = se.scorer.localise(se.dbatch, se.feats, se.counts, off, pep, z, per_candidate=per_candidate)
    if not per_candidate:
        return got, None
    slots, cnt = got
    assert len(cnt) == len(pep)
    return slots, {s: cnt[int(off[s]):int(off[s + 1])] for s in order}


def _hold(se, sr, lists, slots, cnt, state_of, charges=None, ctx=""):
    """every listed slot against the restatement; state_of(i, r) -> (masses, intensities).  Returns the restated records."""
    want = {}
    for slot, peps in lists.items():
        i, r = divmod(slot, se.report)
        masses, intens = state_of(i, r)
        z = charges[slot] if charges is not None else [int(se.feats[i, r]["charge"])] * len(peps)
        w = want[slot] = LR.localise(sr, masses, intens, peps, z)
        where = f"{ctx}spectrum {i} rank {r + 1}"
        LR.assert_slot_equal(slots[slot], w, where)
        if cnt is not None:
            LR.assert_counts_equal(cnt[slot], w["counts"], where)
    # slots without a list: nothing but the marks of "none"
    for slot in set(range(len(slots))) - set(lists):
        s = slots[slot]
        assert int(s["best"]) == int(s["second"]) == LR.NONE and math.isnan(s["ascore"]) and s["n_site_items"] == 0 and s["depth"] == 0
    return want


def _own_and_isomers(se, groups):
    lists = {}
    for i in range(se.dbatch.n):
        for r in range(int(se.counts[i])):
            pep = int(se.feats[i, r]["peptide_idx"])
            others = IR.others(groups, pep)
            if others:
                lists[i * se.report + r] = [pep] + others
    return lists


def test_every_psm_with_isomers(world):
    params = ScorerParams(report_psms=2)
    batch = world.spectra(200, 33)
    se = Search(world, params, batch)
    sr = IR.second_scorer(world.host, world.dbp, params)
    lists = _own_and_isomers(se, world.groups)
    slots, cnt = _localise(se, lists)

    def state(i, r):
        s = SR.spectrum_of(batch, i)
        return s["masses"], s["intensities"]
    want = _hold(se, sr, lists, slots, cnt, state)
    assert len(lists) > 150
    n_site = sum(w["n_site_items"] > 0 for w in want.values())
    n_pos = sum(w["ascore"] > 0 for w in want.values())
    n_best = sum(w["best"] == 0 for w in want.values())
    assert n_site > 100 and n_pos > 50 and 0 < n_best < len(lists), (n_site, n_pos, n_best)
    # NULL for per_candidate: the same records
    again, none = _localise(se, lists, per_candidate=False)
    assert none is None and again.tobytes() == slots.tobytes()
    call_ms, kernel_ms = se.scorer.last_localise_timing()
    assert call_ms > 0.0 and 0.0 < kernel_ms <= call_ms


def test_chimera_ranks_see_the_spectrum_after_peak_removal(world):
    params = ScorerParams(chimera=True, report_psms=3, min_matched_peaks=1)
    batch = world.spectra(200, 34, chimeric=2)
    se = Search(world, params, batch)
    sr = IR.second_scorer(world.host, world.dbp, params)
    lists = _own_and_isomers(se, world.groups)
    slots, cnt = _localise(se, lists)
    states = {}

    def state(i, r):
        if i not in states:
            states[i] = _psm_states(sr, batch, se, i)
        return states[i][r]
    _hold(se, sr, lists, slots, cnt, state)
    later = [s for s in lists if s % 3 > 0]
    changed = [s for s in later if len(state(s // 3, s % 3)[0]) < len(state(s // 3, 0)[0])]
    assert len(later) > 30 and len(changed) == len(later), (len(later), len(changed))
    # and a rank whose own slot has no list still loses its peaks before the next one: some spectrum lists rank 2 but not rank 1
    assert any(s % 3 > 0 and s - 1 not in lists for s in lists)


def test_trip_boundaries_of_64_65_and_129_items(gpu_required):
    """One ion kind, so that a candidate's (ion, fragment charge) items fill exactly 64 (32 ions x 2 charges), 65 (13 x 5) and
    2 x 64 + 1 (43 x 3) lanes; each spectrum holds three in four of the fragments of one placement at every charge, and its list
    is that placement's whole group."""
    w = World(dict(IR.PHOSPHO_DB, ion_kinds=["y"]), fasta=(40, 21))
    params = ScorerParams(report_psms=1, min_matched_peaks=1)
    sr = IR.second_scorer(w.host, w.dbp, params)
    group_of, group_off, members = w.groups
    lens = np.diff(w.host.seq_off.astype(np.int64))
    first = members[group_off[:-1].astype(np.int64)]
    shapes = [(33, 3, 64), (14, 6, 65), (44, 4, 129)]  # peptide length, precursor charge -> items
    rng = np.random.default_rng(3)
    spectra, lists, charges = [], {}, {}
    for k, (n, z, items) in enumerate(shapes):
        assert (n - 1) * (SR.max_fragment_charge(None, z) - 1) == items
        g = int(np.flatnonzero((lens[first] == n) & (w.host.decoy[first] == 0))[0])
        mem = [int(p) for p in members[int(group_off[g]):int(group_off[g + 1])]]
        m, it = _planted(sr, mem[-1], z - 1, keep=lambda size: rng.random(size) < 0.75)
        spectra.append(_spectrum(m, it, w.host.pep_mono[mem[-1]], min(z, 4), k))
        lists[k], charges[k] = mem, [z] * len(mem)
    batch = SpectrumBatch.from_spectra(spectra)
    se = Search(w, params, batch)
    assert np.all(se.counts == 1)
    slots, cnt = _localise(se, lists, charges)

    def state(i, r):
        s = SR.spectrum_of(batch, i)
        return s["masses"], s["intensities"]
    want = _hold(se, sr, lists, slots, cnt, state, charges)
    for k, (_, _, items) in enumerate(shapes):
        assert want[k]["counts"][0][1] == items
        assert want[k]["best"] == len(lists[k]) - 1 and want[k]["counts"][-1][0][9] > 0.5 * items  # matches in the first and the last trip


def test_group_sizes_peak_counts_and_a_single_candidate(world):
    params = ScorerParams(report_psms=3, min_matched_peaks=1)
    sr = IR.second_scorer(world.host, world.dbp, params)
    batch, pair, large, some = _crafted_batch(world, sr)
    se = Search(world, params, batch)
    assert se.counts[0] >= 1 and se.counts[1] == 0 and se.counts[2] >= 1 and se.counts[3] >= 1
    assert [int(batch.peak_off[k + 1] - batch.peak_off[k]) for k in (3, 4)] == [1, 37] and se.counts[4] >= 1 and se.counts[5] >= 1
    lists = _own_and_isomers(se, world.groups)
    # the spectra of 1 and of 37 peaks: the placements of the peptide they were made from, whatever the search reported
    lists[3 * 3] = lists[4 * 3] = [some] + IR.others(world.groups, some)
    sizes = {s: len(v) for s, v in lists.items()}
    assert sizes[0] == 2 and sizes[2 * 3] == 120 and sizes[3 * 3] >= 3, sizes  # groups of 2 and of 120
    single = 5 * 3  # one slot with a single candidate
    lists[single] = [some]
    slots, cnt = _localise(se, lists)

    def state(i, r):
        s = SR.spectrum_of(batch, i)
        return s["masses"], s["intensities"]
    want = _hold(se, sr, lists, slots, cnt, state)
    s = slots[single]
    assert (int(s["best"]), int(s["second"]), int(s["n_site_items"]), int(s["depth"])) == (0, LR.NONE, 0, 0) and math.isnan(s["ascore"])
    assert s["best_score"] > 0.0 and s["second_score"] == 0.0 and not s["a"].any() and not s["b"].any()
    # planted: every fragment of the pair's first member — it is the best placement and the Ascore is positive
    assert want[0]["ascore"] > 0.0 and lists[0][want[0]["best"]] == pair
    # no candidate at all: nothing launched
    empty = se.scorer.localise(se.dbatch, se.feats, se.counts, np.zeros(batch.n * 3 + 1, np.uint64), np.zeros(0, np.uint32))
    assert np.all(empty["best"] == LR.NONE) and se.scorer.last_localise_timing() == (0.0, 0.0)


def test_a_spectrum_that_preprocessing_left_without_peaks(world):
    params = ScorerParams(report_psms=1)
    raws = synthetic_spectra(world.host, 6, 35, varmod_frac=0.9, varmod_residues="STYM", pure_noise_frac=0.0)
    short = raws[2]
    raws[2] = RawSpectrum(short.mz[:9], short.intensity[:9], short.precursor_mz, short.precursor_charge, None, 0.02, None, 0, "short")
    scorer = Scorer(world.dev, params)
    dbatch, kept = scorer.process_upload(RawBatch(raws), 150, True, 0.0, 15)
    se = Search(world, params, dbatch=dbatch, scorer=scorer)
    off, masses, intens, _ = dbatch.download()
    assert off[3] == off[2] and se.counts[2] == 0
    sr = IR.second_scorer(world.host, world.dbp, params)
    lists = _own_and_isomers(se, world.groups)
    assert min(lists) < 2 < max(lists)
    slots, cnt = _localise(se, lists)
    _hold(se, sr, lists, slots, cnt, lambda i, r: (masses[int(off[i]):int(off[i + 1])], intens[int(off[i]):int(off[i + 1])]))


def test_a_spectrum_beyond_64_kb_of_lds(world):
    """7 000 peaks are 77 000 bytes of dynamic LDS, and windows of some 250 peaks each: most ranks are stored as 11"""
    params = ScorerParams(report_psms=1)
    sr = IR.second_scorer(world.host, world.dbp, params)
    _, group_off, members = world.groups
    sizes = np.diff(group_off.astype(np.int64))
    lens = np.diff(world.host.seq_off.astype(np.int64))
    first = members[group_off[:-1].astype(np.int64)]
    pep = int(first[np.flatnonzero((sizes >= 3) & (world.host.decoy[first] == 0) & (lens[first] >= 20))[0]])
    m, it = _planted(sr, pep, 1, base=50000.0)
    it = (it - np.float32(49000.0) * (np.arange(len(it)) % 3 == 0)).astype(np.float32)  # (a third of the planted peaks among the noise's ranks)
    rng = np.random.default_rng(6)
    noise = np.setdiff1d(np.unique(rng.uniform(150.0, 3000.0, 7200).astype(np.float32)), m)[:7000 - len(m)]
    masses = np.concatenate([m, noise])
    intens = np.concatenate([it, rng.lognormal(7.0, 1.0, len(noise)).astype(np.float32)])
    order = np.argsort(masses, kind="stable")
    batch = SpectrumBatch.from_spectra([_spectrum(masses[order], intens[order], world.host.pep_mono[pep], 2, 0)])
    assert int(batch.peak_off[1]) == 7000 and 7000 * 11 > 64 * 1024
    se = Search(world, params, batch)
    assert se.counts[0] == 1
    lists = _own_and_isomers(se, world.groups)
    assert len(lists[0]) >= 3
    slots, cnt = _localise(se, lists)
    want = _hold(se, sr, lists, slots, cnt, lambda i, r: (batch.masses, batch.intensities))
    n_best = want[0]["counts"][want[0]["best"]][0]
    assert 0 < n_best[0] < n_best[9] < want[0]["counts"][0][1]  # the depths differ, and some item is matched at no depth


def test_more_than_eleven_peaks_in_a_window_and_tied_intensities(world):
    """The fragments of one placement among noise of 30 peaks per 100-window whose intensities repeat the fragments' own: ranks
    beyond 11, ties inside a window decided by position"""
    params = ScorerParams(report_psms=1, min_matched_peaks=1)
    sr = IR.second_scorer(world.host, world.dbp, params)
    _, group_off, members = world.groups
    sizes = np.diff(group_off.astype(np.int64))
    lens = np.diff(world.host.seq_off.astype(np.int64))
    first = members[group_off[:-1].astype(np.int64)]
    pep = int(first[np.flatnonzero((sizes >= 3) & (sizes <= 12) & (world.host.decoy[first] == 0) & (lens[first] >= 15))[0]])
    m, _ = _planted(sr, pep, 1)
    it = (np.float32(100.0) + np.arange(len(m), dtype=np.float32) % np.float32(4.0)).astype(np.float32)  # four levels: ties
    rng = np.random.default_rng(9)
    top = int(m.max() // 100) + 1
    noise = np.setdiff1d(np.unique(np.concatenate([rng.uniform(100.0 * w, 100.0 * w + 100.0, 30) for w in range(1, top)]).astype(np.float32)), m)
    masses = np.concatenate([m, noise])
    intens = np.concatenate([it, (np.float32(98.0) + rng.integers(0, 6, len(noise)).astype(np.float32)).astype(np.float32)])
    order = np.argsort(masses, kind="stable")
    batch = SpectrumBatch.from_spectra([_spectrum(masses[order], intens[order], world.host.pep_mono[pep], 2, 0)])
    ranks = LR.depth_ranks(batch.masses, batch.intensities)
    assert (ranks == 11).sum() > 100 and len(np.unique(batch.intensities)) <= 8
    se = Search(world, params, batch)
    assert se.counts[0] == 1
    lists = _own_and_isomers(se, world.groups)
    slots, cnt = _localise(se, lists)
    want = _hold(se, sr, lists, slots, cnt, lambda i, r: (batch.masses, batch.intensities))
    n_best = want[0]["counts"][want[0]["best"]][0]
    assert n_best[0] < n_best[4] < n_best[9]  # ties push fragments down the ranks: the counts grow with the depth


def test_three_ion_kinds(gpu_required):
    w = World(dict(IR.PHOSPHO_DB, ion_kinds=["a", "b", "y"]), fasta=(40, 21))
    params = ScorerParams(report_psms=2)
    batch = w.spectra(60, 32)
    se = Search(w, params, batch)
    sr = IR.second_scorer(w.host, w.dbp, params)
    lists = _own_and_isomers(se, w.groups)
    assert len(lists) > 30
    slots, cnt = _localise(se, lists)

    def state(i, r):
        s = SR.spectrum_of(batch, i)
        return s["masses"], s["intensities"]
    want = _hold(se, sr, lists, slots, cnt, state)
    for slot, wv in want.items():
        i, r = divmod(slot, 2)
        n_res = int(w.host.seq_off[lists[slot][0] + 1] - w.host.seq_off[lists[slot][0]])
        assert wv["counts"][0][1] == 3 * (n_res - 1) * (SR.max_fragment_charge(None, int(se.feats[i, r]["charge"])) - 1)


def test_refused_input(world):
    params = ScorerParams(report_psms=2)
    batch = world.spectra(40, 36)
    se = Search(world, params, batch)
    with_psm = int(np.flatnonzero(se.counts == 1)[0])  # one PSM: slot 1 of the spectrum holds none
    pep = int(se.feats[with_psm, 0]["peptide_idx"])
    lens = np.diff(world.host.seq_off.astype(np.int64))
    other_len = int(np.flatnonzero(lens != lens[pep])[0])
    n_slots = batch.n * 2

    def call(off, peps, charges=None):
        return se.scorer.localise(se.dbatch, se.feats, se.counts, np.asarray(off, np.uint64), np.asarray(peps, np.uint32), charges)

    good = np.zeros(n_slots + 1, np.uint64)
    good[with_psm * 2 + 1:] = 2
    before = call(good, [pep, pep])
    beyond = np.zeros(n_slots + 1, np.uint64)
    beyond[with_psm * 2 + 2:] = 1  # a list on slot 1, beyond counts[i] == 1
    z = int(se.feats[with_psm, 0]["charge"])
    for name, args in [("unequal lengths", (good, [pep, other_len])), ("slot beyond counts", (beyond, [pep])),
                       ("peptide index n_peptides", (good, [pep, world.host.n_peptides])),
                       ("unequal fragment charges", (good, [pep, pep], [2, 4])), ("charge 255", (good, [pep, pep], [z, 255]))]:
        with pytest.raises(L.SageHipError, match="status 1") as err:
            call(*args)
        assert "sage_hip_localise_resident" in str(err.value), name
        assert se.scorer.last_localise_timing() == (0.0, 0.0), name  # nothing was launched
    after = call(good, [pep, pep])
    assert before.tobytes() == after.tobytes()
    s = after[with_psm * 2]
    assert (int(s["best"]), int(s["second"]), int(s["n_site_items"]), int(s["depth"]), float(s["ascore"])) == (0, 1, 0, 1, 0.0)
    assert s["best_score"] == s["second_score"] > 0.0
    feats, counts = se.scorer.score_resident(se.dbatch)
    assert np.array_equal(counts, se.counts) and feats[with_psm, 0].tobytes() == se.feats[with_psm, 0].tobytes()


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def _restated_rows(host, dbp, cfg, files, result_rows, hdr):
    """localisation.sage.tsv from the restatement: the files' spectra processed on the host, searched through the API for the
    PSMs (psm_id counts them in (file, spectrum, rank) order from 1), every placement localised by tests/localise_reference.py"""
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
                others = IR.others(groups, int(f["peptide_idx"]))
                if others:
                    peps = [int(f["peptide_idx"])] + others
                    w = LR.localise(sr, s["masses"], s["intensities"], peps, [int(f["charge"])] * len(peps))
                    by_id[psm_id] = (host.peptide_string(peps[0]), len(peps), host.peptide_string(peps[w["best"]]), w["best_score"],
                                     host.peptide_string(peps[w["second"]]), w["second_score"], w["n_site_items"], w["depth"], w["ascore"],
                                     "true" if w["best"] == 0 else "false")
                psm_id += 1
    ids = [int(r[hdr.index("psm_id")]) for r in result_rows]
    return [(i,) + by_id[i] for i in ids if i in by_id]


def _assert_localisation_file(path, want):
    hdr, rows = _read_tsv(path)
    assert hdr == output.LOCALISATION_HEADERS
    assert len(rows) == len(want)
    for r, w in zip(rows, want):
        assert (int(r[0]), r[1], int(r[2]), r[3], r[5], int(r[7]), int(r[8]), r[10]) == (w[0], w[1], w[2], w[3], w[5], w[7], w[8], w[10]), (r, w)
        for at in (4, 6, 9):
            assert LR.close(float(r[at]), w[at]), (r, w)
            assert r[at] == output.ryu_f64(float(r[at]))


@pytest.mark.parametrize("flow", ["plain", "devices_0_0", "prefilter"])
def test_cli_writes_localisation_and_changes_nothing_else(tmp_path, gpu_required, flow):
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
           "annotate_matches": True, "mzml_paths": files, "score_isomers": True}
    kw = dict(devices=[0, 0]) if flow == "devices_0_0" else {}
    plain, loc = str(tmp_path / "plain"), str(tmp_path / "loc")
    s0 = cli.run(cfg, files, plain, log=lambda m: None, write_pin=True, **kw)
    s1 = cli.run(dict(cfg, localise=True), files, loc, log=lambda m: None, write_pin=True, **kw)
    # without the key: no file, no new summary keys; with it: one more path behind the isomers', every other file byte for byte
    assert not os.path.exists(os.path.join(plain, "localisation.sage.tsv"))
    assert set(s1) - set(s0) == {"localisation_rows", "localisation_ms"}
    lp, ip = os.path.join(loc, "localisation.sage.tsv"), os.path.join(loc, "isomers.sage.tsv")
    at = s1["output_paths"].index(ip)
    assert s1["output_paths"][at + 1] == lp
    assert [p for p in s1["output_paths"] if p != lp] == [p.replace(plain, loc) for p in s0["output_paths"]]
    assert json.load(open(os.path.join(loc, "results.json")))["output_paths"] == s1["output_paths"]
    for name in ("results.sage.tsv", "matched_fragments.sage.tsv", "results.sage.pin", "isomers.sage.tsv"):
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(loc, name), "rb").read(), name
    host = full
    if flow == "prefilter":  # the database the search ran on: the peptides the first pass kept
        sp = cli.search_parameters(cfg)
        host = cli.prefilter_peptides(dbp, fasta, 16, dbp.num_targets(fasta), sp, files, SpectrumProcessor(150, True, 0.0), 0, False,
                                      lambda m: None)
        assert 0 < host.n_peptides < full.n_peptides
    hdr, rows = _read_tsv(os.path.join(loc, "results.sage.tsv"))
    want = _restated_rows(host, dbp, cfg, files, rows, hdr)
    assert s1["localisation_rows"] == s1["isomer_rows"] == len(want) > 20
    _assert_localisation_file(lp, want)
    if flow == "plain":  # the key on its own: the same file, and no isomers.sage.tsv
        alone = str(tmp_path / "alone")
        s2 = cli.run(dict({k: v for k, v in cfg.items() if k != "score_isomers"}, localise=True), files, alone, log=lambda m: None)
        assert open(os.path.join(alone, "localisation.sage.tsv"), "rb").read() == open(lp, "rb").read()
        assert not os.path.exists(os.path.join(alone, "isomers.sage.tsv")) and "isomer_rows" not in s2
