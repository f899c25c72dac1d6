"""The rescoring prune (kernels.hip: score_candidates drops a candidate that cannot reach min_matched_peaks any more,
rescore_spectrum leaves when no candidate reached it) against the same kernels with both switched off
(SAGE_HIP_DEBUG_FLAGS=4096, read when the scorer is created) and against the oracle: the same records, byte for byte.

The cases cannot pass vacuously: `prune_census` counts, from the oracle alone (initial_hits + brute_force), the candidates
whose exact number of matches stays below min_matched_peaks, the spectra in which no candidate reaches it and the spectra in which
a candidate that reaches it stands beside ones that do not; the counters of the profiling instance (SAGE_HIP_PHASE_CLOCKS=1,
sage_hip_debug_prune_counters) must show all three on the device.  (A candidate is pruned when its matches so far
plus the items the peak bitmap lets through stay below the bound: the exact count plus the bitmap's false positives, about one
bin in two hundred.  The main world holds hundreds of candidates with no more than one match where four are asked for.)"""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

from parity_utils import assert_features_equal
from sage_amd import _lib as L
from sage_amd.api import DatabaseParameters, Scorer, ScorerParams, Tolerance
from sage_amd.synthetic import synthetic_fasta
from test_gpu_parity import World

pytestmark = pytest.mark.gpu

PRUNE_OFF = 4096  # SAGE_HIP_DEBUG_FLAGS: the prune and the early leave off
ENZYME = dict(missed_cleavages=1, cleave_at="KR", restrict="P")


def same_psms(fa, ca, fb, cb):
    """(features[n, report_psms], counts[n]) twice: the same records, byte for byte (slots beyond counts[i] belong to no result)"""
    if not np.array_equal(ca, cb):
        return False
    valid = np.arange(fa.shape[1])[None, :] < ca[:, None]
    return fa[valid].tobytes() == fb[valid].tobytes()


def prune_census(orc, params, batch, every=1):
    """From the oracle alone: for every `every`-th spectrum the exact matched_b + matched_y of each candidate of its preliminary
    list.  Returns (candidates below min_matched_peaks, spectra with candidates of which none reaches it, spectra in which a
    candidate that reaches it stands beside one with at most one match)."""
    below = nobody = mixed = 0
    for i in range(0, batch.n, every):
        packed, _, _ = orc.initial_hits(params, batch, i)
        matched = []
        windows = {}
        for word in packed:
            word = int(word)
            pep, z, iso = (word >> 16) & 0xFFFFFFFF, (word >> 8) & 0xFF, (word & 0xFF) - 128
            if pep == 0xFFFFFFFF or (word >> 48) == 0:
                continue
            if (z, iso) not in windows:
                p, m, _ = orc.brute_force(params, batch, i, z, iso)
                windows[(z, iso)] = dict(zip(p.tolist(), m.tolist()))
            matched.append(windows[(z, iso)][pep])
        if not matched:
            continue
        matched = np.array(matched)
        below += int((matched < params.min_matched_peaks).sum())
        if matched.max() < params.min_matched_peaks:
            nobody += 1
        elif matched.min() + 3 <= params.min_matched_peaks:
            mixed += 1
    return below, nobody, mixed


def run(world, batch, params, monkeypatch, flags=0, general=False, clocks=False):
    for var in ("SAGE_HIP_RESCORE_GENERAL", "SAGE_HIP_DEBUG_FLAGS", "SAGE_HIP_PHASE_CLOCKS"):
        monkeypatch.delenv(var, raising=False)
    if general:
        monkeypatch.setenv("SAGE_HIP_RESCORE_GENERAL", "1")
    if flags:
        monkeypatch.setenv("SAGE_HIP_DEBUG_FLAGS", str(flags))
    if clocks:
        monkeypatch.setenv("SAGE_HIP_PHASE_CLOCKS", "1")
    scorer = Scorer(world.dev, params)  # (the three variables are read here, once)
    for var in ("SAGE_HIP_RESCORE_GENERAL", "SAGE_HIP_DEBUG_FLAGS", "SAGE_HIP_PHASE_CLOCKS"):
        monkeypatch.delenv(var, raising=False)
    gf, gc = scorer.score_resident(scorer.upload(batch))
    gf, gc = gf.copy(), gc.copy()
    counters = None
    if clocks:
        out = np.zeros(4, np.uint64)
        L.check(L.load().sage_hip_debug_prune_counters(scorer._h, L.as_ptr(out, C.c_uint64)))
        counters = dict(zip(("candidates", "items", "left_early", "mixed"), (int(v) for v in out)))
    scorer.close()
    return gf, gc, counters


def check(world, batch, params, monkeypatch, ctx, flag_sets=(0,), instances=(False,), want_psms=True):
    """prune on / off, for every route in flag_sets x instances: equal to each other and to the oracle.  Returns the oracle's PSM count."""
    of, oc, _, _ = world.orc.score(params, batch)
    n = None
    for general in instances:
        for flags in flag_sets:
            c = f"{ctx}, flags={flags}, general={general}"
            nf, nc, _ = run(world, batch, params, monkeypatch, flags, general)
            pf, pc, _ = run(world, batch, params, monkeypatch, flags | PRUNE_OFF, general)
            assert same_psms(nf, nc, pf, pc), f"{c}: the prune changed the records"
            n = assert_features_equal(nf, nc, of, oc, c + " (prune on)")
            assert assert_features_equal(pf, pc, of, oc, c + " (prune off)") == n
            assert (n > 0) == want_psms, c
    return n


@pytest.fixture(scope="module")
def worlds(gpu_required):
    # C3-like: known charges, +-10 ppm, windows of a handful of candidates
    narrow = World(synthetic_fasta(300, seed=11),
                   DatabaseParameters(bucket_size=2048, enzyme=ENZYME, static_mods={"C": 57.0215}, variable_mods={"M": [15.9949]}),
                   {}, 600, seed=21)
    # tie-rich: every peptide beside its isoleucine / leucine twin (equal masses and fragments: equal hyperscores at the top)
    fasta = synthetic_fasta(60, seed=17)
    twin = fasta.replace("I", "#").replace("L", "I").replace("#", "L").replace(">sp|SYN", ">sp|TWN")
    ties = World(fasta + twin, DatabaseParameters(bucket_size=1024, enzyme=ENZYME, static_mods={"C": 57.0215}), {}, 300, seed=29)
    return {
        "narrow": (narrow, narrow.batch, {}),
        "ties": (ties, ties.batch, dict(precursor_tol=Tolerance("da", -20.0, 20.0))),
        "open": (narrow, narrow.batch.subset(np.arange(0, narrow.batch.n, 3)), dict(precursor_tol=Tolerance("da", -200.0, 200.0))),
    }


@pytest.fixture(scope="module")
def long_world(gpu_required):
    # peptides of 34..70 residues only: 2 x (L - 1) > 64 ions, so every candidate is scored in two or three chunks and judged on its last
    return World(synthetic_fasta(120, seed=41),
                 DatabaseParameters(bucket_size=1024, enzyme=dict(missed_cleavages=2, min_len=34, max_len=70, cleave_at="KR", restrict="P"),
                                    peptide_max_mass=9000.0, static_mods={"C": 57.0215}), {}, 200, seed=43)


@pytest.fixture(scope="module")
def high_charge_world(gpu_required):
    # precursor charges 5 and 6 with max_fragment_charge None: four and five fragment charges per ion — the bitmap filters three
    return World(synthetic_fasta(150, seed=47),
                 DatabaseParameters(bucket_size=1024, enzyme=dict(missed_cleavages=2, cleave_at="KR", restrict="P"), static_mods={"C": 57.0215}),
                 dict(charges=((5, 0.5), (6, 0.5))), 200, seed=53)


@pytest.mark.parametrize("report_psms", [1, 5])
@pytest.mark.parametrize("name", ["narrow", "ties", "open"])
def test_prune_on_and_off_on_both_instances(worlds, monkeypatch, name, report_psms):
    """the three worlds x report_psms 1 and 5, the dense list (0), the walk (128), the list capped at 64 items (256), both instances"""
    world, batch, kw = worlds[name]
    check(world, batch, ScorerParams(report_psms=report_psms, **kw), monkeypatch, f"{name}, report_psms={report_psms}",
          flag_sets=(0, 128, 256), instances=(False, True))


@pytest.mark.parametrize("min_matched_peaks", [1, 4, 6, 1000])
@pytest.mark.parametrize("name", ["narrow", "open"])
def test_min_matched_peaks_values(worlds, monkeypatch, name, min_matched_peaks):
    """1 prunes nothing that has a hit; 1000 is a value no candidate reaches: every spectrum leaves early, no record"""
    world, batch, kw = worlds[name]
    for report_psms in (1, 5):
        params = ScorerParams(report_psms=report_psms, min_matched_peaks=min_matched_peaks, **kw)
        check(world, batch, params, monkeypatch, f"{name}, min_matched_peaks={min_matched_peaks}, report_psms={report_psms}",
              flag_sets=(0, 128), instances=(False, True), want_psms=min_matched_peaks != 1000)


@pytest.mark.parametrize("name", ["narrow", "ties", "open"])
def test_chimera_rounds(worlds, monkeypatch, name):
    """every round judged on its own, against the round-0 bitmap (a superset of the remaining peaks' bins)"""
    world, batch, kw = worlds[name]
    for min_matched_peaks in (4, 6):
        check(world, batch, ScorerParams(chimera=True, report_psms=3, min_matched_peaks=min_matched_peaks, **kw), monkeypatch,
              f"{name}, chimera, min_matched_peaks={min_matched_peaks}", flag_sets=(0, 128))


def test_candidates_of_several_chunks(long_world, monkeypatch):
    w = long_world
    lens = np.diff(w.host.seq_off.astype(np.int64))
    assert int(lens.min()) >= 34 and int(lens.max()) > 34
    for kw in (dict(), dict(report_psms=5, precursor_tol=Tolerance("da", -50.0, 50.0)),
               dict(min_matched_peaks=8, precursor_tol=Tolerance("da", -50.0, 50.0)),
               dict(chimera=True, report_psms=2, precursor_tol=Tolerance("da", -50.0, 50.0))):
        check(w, w.batch, ScorerParams(**kw), monkeypatch, f"long peptides, {kw}", flag_sets=(0, 128, 256), instances=(False, True))


def test_more_than_three_fragment_charges(high_charge_world, monkeypatch):
    """nfz > 3: the masks hold every ion of the chunk and an ion makes more than three items — such a candidate is never pruned"""
    w = high_charge_world
    assert int(np.min(w.batch.precursor_charge)) >= 5
    for kw in (dict(max_fragment_charge=None), dict(max_fragment_charge=None, report_psms=5, min_matched_peaks=6,
                                                    precursor_tol=Tolerance("da", -30.0, 30.0)),
               dict(max_fragment_charge=3, precursor_tol=Tolerance("da", -30.0, 30.0))):
        check(w, w.batch, ScorerParams(**kw), monkeypatch, f"charges 5 and 6, {kw}", flag_sets=(0, 128), instances=(False, True))


def test_fragment_tolerance_that_sets_every_bin(worlds, monkeypatch):
    """a reach above 4 Da switches the filter off (build_peak_bitmap sets every bin): the bound is the number of items, nothing wrong is pruned"""
    world, batch, kw = worlds["narrow"]
    for min_matched_peaks in (4, 30):
        check(world, batch, ScorerParams(fragment_tol=Tolerance("da", -5.0, 5.0), min_matched_peaks=min_matched_peaks, **kw), monkeypatch,
              f"fragment_tol +-5 Da, min_matched_peaks={min_matched_peaks}", flag_sets=(0, 128), instances=(False, True))


def test_the_prune_really_happens(worlds, monkeypatch):
    """The main world: the oracle says what there is to prune, the profiling instance's counters say it was pruned."""
    world, batch, kw = worlds["narrow"]
    params = ScorerParams(**kw)
    assert params.min_matched_peaks == 4 and params.report_psms == 1
    below, nobody, mixed = prune_census(world.orc, params, batch)
    print(f"oracle: {below} candidates below min_matched_peaks, {nobody} spectra in which nobody passes, {mixed} mixed spectra")
    # (the early leave hangs on exact counts alone: one such spectrum is enough; the other two leave room for the bitmap's false positives)
    assert below >= 200 and nobody >= 1 and mixed >= 20, (below, nobody, mixed)
    of, oc, _, _ = world.orc.score(params, batch)
    for general in (False, True):
        gf, gc, on = run(world, batch, params, monkeypatch, 0, general, clocks=True)
        pf, pc, off = run(world, batch, params, monkeypatch, PRUNE_OFF, general, clocks=True)
        print(f"general={general}: counters with the prune on {on}, off {off}")
        assert assert_features_equal(gf, gc, of, oc, f"profiling instance, general={general}") > 0
        assert same_psms(gf, gc, pf, pc)
        assert on["candidates"] >= 1 and on["items"] >= on["candidates"]
        assert on["candidates"] <= 2 * below  # (only candidates that cannot pass; a spectrum is rescored at most twice: the retry pass)
        assert on["left_early"] >= 1 and on["mixed"] >= 1
        assert off == dict(candidates=0, items=0, left_early=0, mixed=0)
    # a bound nobody reaches: every spectrum with a list leaves early, nothing is reported
    gf, gc, on = run(world, batch, replace(params, min_matched_peaks=1000), monkeypatch, 0, False, clocks=True)
    assert int(gc.sum()) == 0 and on["left_early"] >= nobody and on["mixed"] == 0
