"""The flat route of the peak-bitmap filter (kernels.hip: score_candidates deals the candidates' ions, in octets, to all 64 lanes;
core.h: flat_octets ...) against the per-lane filter (SAGE_HIP_DEBUG_FLAGS=8192, read when the scorer is created) and against the
oracle: the same records, byte for byte.  Three settings per case: the default (the wave-uniform choice between the routes), the flat
route wherever its bytes fit (16384) and the per-lane filter alone (8192).

The flat route belongs to the instance without chimera rounds (and to rescore_big_kernel's short-list instance); the general
instance — chimera searches, SAGE_HIP_RESCORE_GENERAL=1 — keeps to the per-lane filter under every setting (kernels.hip:
rescore_spectrum instantiates score_candidates with FLAT = !CHIMERA), and must give the same records.

The cases cannot pass vacuously: the counters of the profiling instance (SAGE_HIP_PHASE_CLOCKS=1, sage_hip_debug_filter_counters)
must show flat chunks and trips where the route is meant to be taken, none with 8192, and fewer flat trips than the per-lane
filter's where the lists are short."""
import ctypes as C

import numpy as np
import pytest

from parity_utils import assert_features_equal
from sage_amd import _lib as L
from sage_amd.api import DatabaseParameters, Scorer, ScorerParams, Tolerance
from sage_amd.synthetic import synthetic_fasta
from test_gpu_parity import World

pytestmark = pytest.mark.gpu

PER_LANE = 8192     # SAGE_HIP_DEBUG_FLAGS: the per-lane filter for every chunk
FLAT_ALWAYS = 16384  # ... the flat route for every chunk whose bytes fit the area
ENZYME = dict(missed_cleavages=1, cleave_at="KR", restrict="P")
ENV = ("SAGE_HIP_RESCORE_GENERAL", "SAGE_HIP_DEBUG_FLAGS", "SAGE_HIP_PHASE_CLOCKS")


def same_psms(fa, ca, fb, cb):
    """(features[n, report_psms], counts[n]) twice: the same records, byte for byte (slots beyond counts[i] belong to no result)"""
    if not np.array_equal(ca, cb):
        return False
    valid = np.arange(fa.shape[1])[None, :] < ca[:, None]
    return fa[valid].tobytes() == fb[valid].tobytes()


def run(world, batch, params, monkeypatch, flags=0, general=False, clocks=False):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    if general:
        monkeypatch.setenv("SAGE_HIP_RESCORE_GENERAL", "1")
    if flags:
        monkeypatch.setenv("SAGE_HIP_DEBUG_FLAGS", str(flags))
    if clocks:
        monkeypatch.setenv("SAGE_HIP_PHASE_CLOCKS", "1")
    scorer = Scorer(world.dev, params)  # (the three variables are read here, once)
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    gf, gc = scorer.score_resident(scorer.upload(batch))
    gf, gc = gf.copy(), gc.copy()
    counters = None
    if clocks:
        out = np.zeros(4, np.uint64)
        L.check(L.load().sage_hip_debug_filter_counters(scorer._h, L.as_ptr(out, C.c_uint64)))
        counters = dict(zip(("flat_chunks", "flat_trips", "would", "lane_trips"), (int(v) for v in out)))
    scorer.close()
    return gf, gc, counters


def check(world, batch, params, monkeypatch, ctx, flag_sets=(0,), instances=(False,), route=True, of_oc=None):
    """default / flat wherever it fits / per-lane, for every route in flag_sets x instances: equal to each other and to the oracle;
    then the profiling instance's counters: flat trips where `route` says the route is meant to be taken, none under 8192.
    Returns the counters of the default setting and of the forced flat route."""
    of, oc = of_oc if of_oc is not None else world.orc.score(params, batch)[:2]
    for general in instances:
        for flags in flag_sets:
            c = f"{ctx}, flags={flags}, general={general}"
            lf, lc, _ = run(world, batch, params, monkeypatch, flags | PER_LANE, general)
            n = assert_features_equal(lf, lc, of, oc, c + " (per-lane)")
            for extra, what in ((0, "default"), (FLAT_ALWAYS, "flat wherever it fits")):
                ff, fc, _ = run(world, batch, params, monkeypatch, flags | extra, general)
                assert same_psms(ff, fc, lf, lc), f"{c}: the flat route ({what}) changed the records"
                assert assert_features_equal(ff, fc, of, oc, c + f" ({what})") == n
    dflt = forced = None
    for general in instances:
        df, dc, dflt = run(world, batch, params, monkeypatch, flag_sets[0], general, clocks=True)
        ff, fc, forced = run(world, batch, params, monkeypatch, flag_sets[0] | FLAT_ALWAYS, general, clocks=True)
        pf, pc, off = run(world, batch, params, monkeypatch, flag_sets[0] | PER_LANE, general, clocks=True)
        print(f"{ctx}, general={general}: filter counters default {dflt}, flat wherever it fits {forced}, per-lane {off}")
        assert_features_equal(df, dc, of, oc, ctx + " (profiling instance)")
        assert same_psms(df, dc, ff, fc) and same_psms(df, dc, pf, pc), ctx
        assert off["flat_chunks"] == 0 and off["flat_trips"] == 0 and off["lane_trips"] > 0, (ctx, off)
        if general or params.chimera:  # the general instance: the per-lane filter whatever the flags say, and the same trips
            assert dflt == off and forced == off, (ctx, general, dflt, forced, off)
    if instances[-1] or params.chimera:
        return dflt, forced
    assert forced["flat_chunks"] > 0 and forced["flat_trips"] >= forced["flat_chunks"], (ctx, forced)
    assert forced["flat_chunks"] >= dflt["flat_chunks"], (ctx, dflt, forced)
    if route:
        assert dflt["flat_chunks"] > 0 and dflt["flat_trips"] >= dflt["flat_chunks"], (ctx, dflt)
        # (a flat trip tests 8 ions per lane, a per-lane trip 4: the choice takes the route only where it undercuts the longest lane)
        assert 2 * dflt["flat_trips"] < dflt["would"], (ctx, dflt)
    return dflt, forced


def valid_counts(world, params, batch):
    """valid candidates of every spectrum's preliminary list (the oracle's, in the heap's layout), and whether some list has an
    empty slot in front of a valid one"""
    counts, holes = [], False
    for i in range(batch.n):
        packed, _, _ = world.orc.initial_hits(params, batch, i)
        ok = np.array([((int(w) >> 16) & 0xFFFFFFFF) != 0xFFFFFFFF and (int(w) >> 48) != 0 for w in packed], dtype=bool)
        counts.append(int(ok.sum()))
        if ok.any() and not ok[:np.flatnonzero(ok)[-1]].all():
            holes = True
    return np.array(counts), holes


@pytest.fixture(scope="module")
def worlds(gpu_required):
    # C3-like: known charges 2 / 3 / 4 (nfz 1 to 3), +-10 ppm, windows of a handful of candidates
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
def length_world(gpu_required):
    # peptides of 2 .. 70 residues: 2, 8, 64 and 66 ions (2, 5, 33 and 34 residues) and three chunks (70)
    return World(synthetic_fasta(120, seed=41),
                 DatabaseParameters(bucket_size=1024, enzyme=dict(missed_cleavages=2, min_len=2, max_len=70, cleave_at="KR", restrict="P"),
                                    peptide_min_mass=150.0, peptide_max_mass=9000.0, static_mods={"C": 57.0215}), {}, 300, seed=43)


@pytest.fixture(scope="module")
def high_charge_world(gpu_required):
    # precursor charges 4, 5 and 6 with max_fragment_charge None: three (filtered), four and five (unfiltered) fragment charges
    return World(synthetic_fasta(150, seed=47),
                 DatabaseParameters(bucket_size=1024, enzyme=dict(missed_cleavages=2, cleave_at="KR", restrict="P"), static_mods={"C": 57.0215}),
                 dict(charges=((4, 0.4), (5, 0.3), (6, 0.3))), 200, seed=53)


@pytest.mark.parametrize("report_psms", [1, 5])
@pytest.mark.parametrize("name", ["narrow", "ties", "open"])
def test_flat_and_per_lane_on_both_instances(worlds, monkeypatch, name, report_psms):
    """the three worlds x report_psms 1 and 5, the instance without chimera rounds and the general one"""
    world, batch, kw = worlds[name]
    check(world, batch, ScorerParams(report_psms=report_psms, **kw), monkeypatch, f"{name}, report_psms={report_psms}",
          instances=(True, False))


@pytest.mark.parametrize("name", ["narrow", "ties", "open"])
def test_chimera_rounds(worlds, monkeypatch, name):
    """the general instance: every round filters again, per lane; 8192 and 16384 change nothing there"""
    world, batch, kw = worlds[name]
    check(world, batch, ScorerParams(chimera=True, report_psms=3, **kw), monkeypatch, f"{name}, chimera")


@pytest.mark.parametrize("flags", [32, 64, 128, 256, 4096])
def test_routes_behind_the_filter(worlds, monkeypatch, flags):
    """no cooperative path (32), every heavy lane cooperative (64), the walk (128), the dense list capped (256), no prune (4096):
    each sees the same masks from either route"""
    for name in ("narrow", "open"):
        world, batch, kw = worlds[name]
        check(world, batch, ScorerParams(**kw), monkeypatch, name, flag_sets=(flags,))


def test_peptide_lengths(length_world, monkeypatch):
    """2, 8, 64 and 66 ions and three chunks; short candidates beside long ones in one list"""
    w = length_world
    lens = set(np.diff(w.host.seq_off.astype(np.int64)).tolist())
    assert {2, 5, 33, 34, 70} <= lens, sorted(lens)
    for kw in (dict(), dict(report_psms=5, precursor_tol=Tolerance("da", -300.0, 300.0)),
               dict(chimera=True, report_psms=2, precursor_tol=Tolerance("da", -300.0, 300.0))):
        check(w, w.batch, ScorerParams(**kw), monkeypatch, f"peptides of 2 to 70 residues, {kw}", flag_sets=(0, 128),
              instances=(True, False) if not kw.get("chimera") else (False,))


def test_fragment_charges(worlds, high_charge_world, monkeypatch):
    """precursor charges 2, 3, 4 (nfz 1 to 3); 5 and 6 (unfiltered); and lists that mix them (the charge overridden: 2 to 6)"""
    world, batch, kw = worlds["narrow"]
    assert {2, 3, 4} <= set(np.asarray(batch.precursor_charge).tolist())
    w = high_charge_world
    assert {4, 5, 6} <= set(np.asarray(w.batch.precursor_charge).tolist())
    for kw in (dict(max_fragment_charge=None), dict(max_fragment_charge=None, report_psms=5, precursor_tol=Tolerance("da", -30.0, 30.0)),
               dict(max_fragment_charge=3, precursor_tol=Tolerance("da", -30.0, 30.0))):
        check(w, w.batch, ScorerParams(max_precursor_charge=6, **kw), monkeypatch, f"charges 4 to 6, {kw}", instances=(True, False))
    # one list, several precursor charges: lanes with nfz 1, 2, 3 beside lanes with 4 and 5
    mixed = ScorerParams(max_precursor_charge=6, override_precursor_charge=True, max_fragment_charge=None, report_psms=3,
                         precursor_tol=Tolerance("da", -3.0, 3.0))
    sub = w.batch.subset(np.arange(0, w.batch.n, 2))
    check(w, sub, mixed, monkeypatch, "charges 2 to 6 in one list", instances=(True, False))


def test_fragment_tolerance_that_sets_every_bin(worlds, monkeypatch):
    """a reach above 4 Da switches the filter off (build_peak_bitmap sets every bin): every byte of the area comes back 0xFF"""
    world, batch, kw = worlds["narrow"]
    check(world, batch, ScorerParams(fragment_tol=Tolerance("da", -5.0, 5.0), **kw), monkeypatch, "fragment_tol +-5 Da", flag_sets=(0, 128),
          instances=(True, False))


def test_list_lengths(worlds, monkeypatch):
    """lists of 1, 2, 16, 17, 32, 33 and 50 valid candidates, with empty slots between valid ones; the short lists are where the flat
    route saves most"""
    world, batch, _ = worlds["narrow"]
    want = {1, 2, 16, 17, 32, 33, 50}
    picked, found, holes = {}, set(), False
    for da in (0.02, 0.5, 2.0, 5.0, 12.0, 40.0):
        params = ScorerParams(precursor_tol=Tolerance("da", -da, da))
        sub = batch.subset(np.arange(0, batch.n, 4))
        counts, h = valid_counts(world, params, sub)
        idx = np.flatnonzero(np.isin(counts, sorted(want)))
        if len(idx):
            picked[da] = (params, sub.subset(idx), counts[idx])
            found |= set(counts[idx].tolist())
            holes = holes or h
    assert found == want, sorted(found)
    assert holes
    for da, (params, sub, counts) in picked.items():
        check(world, sub, params, monkeypatch, f"lists of {sorted(set(counts.tolist()))} valid candidates (+-{da} Da)", route=False)
    # the short lists alone (16 candidates and fewer): the route is taken, and its trips undercut the per-lane filter's
    params, sub, counts = picked[0.5]
    check(world, sub.subset(np.flatnonzero(counts <= 16)), params, monkeypatch, "lists of at most 16 valid candidates")
