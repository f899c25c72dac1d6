"""The one-trip route of the cooperative path of score_candidates (kernels.hip): a heavy candidate's LAST chunk, where the bitmap's
LDS is free, with at most 64 (ion, fragment charge) items goes through ONE lookup trip — item p on lane p, in the reference's
(ion, charge) order (core.h: coop_item_pos) — and its three sums are made by three lanes over LDS slots.  Every other heavy chunk
keeps the trip per fragment charge and the readlane sums, which is also the independent route: SAGE_HIP_DEBUG_FLAGS=262144 forces
it everywhere.  Per case the records under

    0                       the default choice of heavy candidates, the one-trip route where it applies
    262144                  ... all of them on the trip per charge
    64 | 32768              every candidate from its first hit on the cooperative path: the whole world through the one-trip route
    64 | 32768 | 262144     ... and through the trip per charge
    32                      no cooperative path: the dense list and the walk

are equal byte for byte, and equal to the oracle.  No case passes vacuously: the profiling instance's route counters
(SAGE_HIP_PHASE_CLOCKS=1, sage_hip_debug_heavy_routes: chunks on the one-trip route, chunks on the trip per charge) must show the
route taken where a case says so, fallbacks where a chunk has more than 64 items or is not the last, and nothing on the route
under 262144, in chimera searches and in the general instance (SAGE_HIP_RESCORE_GENERAL=1), which do not carry it."""
import ctypes as C

import numpy as np
import pytest

from parity_utils import assert_features_equal
from sage_amd import _lib as L
from sage_amd.api import RawSpectrum, Scorer, ScorerParams, SpectrumBatch, SpectrumProcessor, Tolerance
from sage_amd.synthetic import _MASS_LUT, PROTON
from test_gpu_rescore_heavy_adds import ENV, high_charge_world, length_world, records, run, worlds  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NO_COOP, EVERY_HEAVY, FIRST_HIT, PER_CHARGE = 32, 64, 32768, 262144
FORCED = EVERY_HEAVY | FIRST_HIT
FLAG_SETS = (0, PER_CHARGE, FORCED, FORCED | PER_CHARGE, NO_COOP)


def run_routes(world, batch, params, monkeypatch, flags, general=False):
    """the profiling instance under `flags`: records and (chunks on the one-trip route, chunks on the trip per charge)"""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    if general:
        monkeypatch.setenv("SAGE_HIP_RESCORE_GENERAL", "1")
    if flags:
        monkeypatch.setenv("SAGE_HIP_DEBUG_FLAGS", str(flags))
    monkeypatch.setenv("SAGE_HIP_PHASE_CLOCKS", "1")
    scorer = Scorer(world.dev, params)
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    gf, gc = scorer.score_resident(scorer.upload(batch))
    rec = records(gf, gc)
    heavy, routes = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    L.check(L.load().sage_hip_debug_heavy_counters(scorer._h, L.as_ptr(heavy, C.c_uint64)))
    L.check(L.load().sage_hip_debug_heavy_routes(scorer._h, L.as_ptr(routes, C.c_uint64)))
    scorer.close()
    assert int(routes.sum()) == int(heavy[0]), (routes, heavy)  # (every heavy chunk took one of the two)
    return rec, (int(routes[0]), int(routes[1]))


def check(world, batch, params, monkeypatch, ctx, general=False, one_trip=True, fallbacks=None, default_flags=False):
    """the five settings against each other and the oracle; then the counters with every candidate on the path (or, default_flags,
    with the kernel's own choice of heavy candidates): on the route iff `one_trip`, fallbacks iff `fallbacks` (None: either), and
    never on the route under 262144.  Returns the (one-trip, per-charge) chunk counts."""
    of, oc = world.orc.score(params, batch)[:2]
    base = None
    for flags in FLAG_SETS:
        gf, gc, _ = run(world, batch, params, monkeypatch, flags, general)
        n = assert_features_equal(gf, gc, of, oc, f"{ctx}, flags={flags}, general={general}")
        if base is None:
            base = records(gf, gc)
            assert n > 0, ctx
        assert records(gf, gc) == base, f"{ctx}, general={general}: flags={flags} changed the records"
    want = 0 if default_flags else FORCED
    rec, routes = run_routes(world, batch, params, monkeypatch, want, general)
    assert rec == base, f"{ctx}: the profiling instance"
    rec, off = run_routes(world, batch, params, monkeypatch, want | PER_CHARGE, general)
    assert rec == base, f"{ctx}: the profiling instance, trip per charge"
    print(f"{ctx}, general={general}: (one-trip, per-charge) chunks {routes}; under 262144 {off}")
    assert off[0] == 0 and off[1] == sum(routes), (ctx, routes, off)
    assert (routes[0] > 0) == bool(one_trip), (ctx, routes)
    if fallbacks is not None:
        assert (routes[1] > 0) == bool(fallbacks), (ctx, routes)
    return routes


@pytest.fixture(scope="module")
def length_worlds(gpu_required):
    return {"by": length_world(["b", "y"]), "abcxyz": length_world(["a", "b", "c", "x", "y", "z"])}


def fragments(host, pep):
    a, b = int(host.seq_off[pep]), int(host.seq_off[pep + 1])
    res = _MASS_LUT[host.seq[a:b]] + host.mods[a:b].astype(np.float64)
    nterm = float(host.nterm[pep]) if not np.isnan(host.nterm[pep]) else 0.0
    bs = nterm + np.cumsum(res)[:-1]
    return bs, float(host.pep_mono[pep]) - bs, float(host.pep_mono[pep])


def crafted(host, recipe, seed, max_peaks=150):
    """recipe: per spectrum (precursor peptide, precursor charge, [(peptide, fragment charge, share of its b / y ions kept)], noise
    peaks).  The listed ladders go in first-come until `max_peaks` peaks are there, so that the processor's cut keeps what was meant."""
    rng = np.random.default_rng(seed)
    spectra = []
    for i, (pep, z, ladders, noise) in enumerate(recipe):
        mono = float(host.pep_mono[pep])
        mz = []
        for p, c, share in ladders:
            bs, ys, _ = fragments(host, p)
            frag = np.concatenate([bs, ys])
            frag = frag[rng.random(len(frag)) < share]
            mz.append((frag + c * PROTON) / c)
        mz = np.concatenate(mz)[:max_peaks - noise]
        mz = mz * (1.0 + rng.normal(0.0, 2.0, len(mz)) * 1e-6)
        it = rng.lognormal(9.0, 0.5, len(mz))
        if noise:
            mz = np.concatenate([mz, rng.uniform(150.0, max(mono, 400.0), noise)])
            it = np.concatenate([it, rng.lognormal(6.0, 1.0, noise)])
        order = np.argsort(mz, kind="stable")
        spectra.append(RawSpectrum(mz[order].astype(np.float32), it[order].astype(np.float32), float(np.float32((mono + z * PROTON) / z)), z, None,
                                   scan_start_time=float(i), file_id=0, id=f"scan={i}"))
    return SpectrumBatch.from_spectra([SpectrumProcessor(max_peaks, False, 0.0).process(r) for r in spectra])


def peptides_of_length(host, n, k):
    lens = np.diff(host.seq_off.astype(np.int64))
    idx = np.flatnonzero((lens == n) & (host.decoy == 0))
    assert len(idx), f"no target peptide of {n} residues"
    return [int(idx[j % len(idx)]) for j in range(k)]


@pytest.mark.parametrize("min_matched_peaks", [1, 4])
@pytest.mark.parametrize("kinds", ["by", "abcxyz"])
def test_peptide_lengths_and_ion_kinds(length_worlds, monkeypatch, kinds, min_matched_peaks):
    """2, 5, 33, 34 and 70 residues (one-bit segments; a full last chunk; a last chunk of two ions behind a full one; three chunks —
    the first two never the last) x two and six ion kinds (alternating n- and c-terminal segments) x the prune's bound 1 and 4;
    precursor charges 2, 3, 4: one to three fragment charges"""
    w = length_worlds[kinds]
    lens = set(np.diff(w.host.seq_off.astype(np.int64)).tolist())
    assert {2, 5, 33, 34, 70} <= lens, sorted(lens)
    assert {2, 3, 4} <= set(np.asarray(w.batch.precursor_charge).tolist())
    check(w, w.batch, ScorerParams(min_matched_peaks=min_matched_peaks), monkeypatch, f"lengths, {kinds}, min_matched_peaks={min_matched_peaks}",
          fallbacks=True)


def test_seventy_residues_fall_back_before_the_last_chunk(length_worlds, monkeypatch):
    """a 70-residue peptide, 138 ions with two kinds: chunks 0 and 1 are not the last (trip per charge), chunk 2 is (one trip)"""
    w = length_worlds["by"]
    peps = peptides_of_length(w.host, 70, 6)
    batch = crafted(w.host, [(p, 2 + i % 3, [(p, 1, 0.7), (p, 2, 0.3)], 30) for i, p in enumerate(peps)], seed=5)
    routes = check(w, batch, ScorerParams(min_matched_peaks=1), monkeypatch, "70 residues", fallbacks=True)
    assert routes[1] >= 2 * len(peps), routes  # (the true peptide's first two chunks in every spectrum)


@pytest.mark.parametrize("kinds", ["by", "abcxyz"])
def test_more_than_64_items_fall_back(length_worlds, monkeypatch, kinds):
    """33 residues (64 b / y ions: ONE chunk, the last) and 34 residues (a full chunk and two ions) against a spectrum that holds the
    peptide's ions at fragment charges 1, 2 and 3, precursor charge 4: the 33-residue peptide's only chunk has about 150 items and
    keeps the trip per charge — under the kernel's own choice of heavy candidates too —, beside sparse spectra of the same peptides,
    whose chunk takes the one trip"""
    w = length_worlds[kinds]
    p33, p34 = peptides_of_length(w.host, 33, 4), peptides_of_length(w.host, 34, 4)
    dense = [(p, 4, [(p, 1, 1.0), (p, 2, 1.0), (p, 3, 1.0)], 0) for p in p33 + p34]
    batch = crafted(w.host, dense, seed=7)
    # the dense spectra alone, the kernel's own choice (more than COOP_MIN_HITS hits): the 33-residue chunks fall back
    of, oc = w.orc.score(ScorerParams(min_matched_peaks=1), batch)[:2]
    rec, routes = run_routes(w, batch, ScorerParams(min_matched_peaks=1), monkeypatch, 0)
    gf, gc, _ = run(w, batch, ScorerParams(min_matched_peaks=1), monkeypatch, NO_COOP)
    assert_features_equal(gf, gc, of, oc, f"dense, {kinds}")
    assert rec == records(gf, gc)
    print(f"dense, {kinds}: default flags (one-trip, per-charge) {routes}")
    assert routes[1] >= len(p33), routes
    # ... and beside sparse spectra of the same peptides, all five settings
    sparse = [(p, 2 + i % 3, [(p, 1, 0.4), (p, 2, 0.15)], 40) for i, p in enumerate(p33 + p34)]
    both = crafted(w.host, dense + sparse, seed=9)
    check(w, both, ScorerParams(min_matched_peaks=1, report_psms=2), monkeypatch, f"dense and sparse, {kinds}", fallbacks=True)


@pytest.mark.parametrize("report_psms", [1, 5])
@pytest.mark.parametrize("min_matched_peaks", [1, 4])
def test_two_heavy_candidates_and_the_dense_list_in_the_same_bytes(length_worlds, monkeypatch, report_psms, min_matched_peaks):
    """+-20 Da around two peptides whose ladders are both in the spectrum: under the kernel's own choice two heavy candidates take the
    route one after the other, the second in the words the first left, and the window's other candidates then go through the dense
    list, which overwrites the same bytes.  (A world without variable modifications: a peptide's modified forms share half its ions,
    and more than COOP_MAX_LANES heavy candidates leave the path.)"""
    w = length_worlds["by"]
    host = w.host
    lens = np.diff(host.seq_off.astype(np.int64))
    ok = np.flatnonzero((host.decoy == 0) & (lens >= 12) & (lens <= 30))
    order = ok[np.argsort(host.pep_mono[ok], kind="stable")]
    gaps = np.diff(host.pep_mono[order].astype(np.float64))
    found = np.flatnonzero((gaps > 0.5) & (gaps < 15.0))
    at = found[:: max(1, len(found) // 12)][:12]  # (a dozen pairs spread over the mass range)
    assert len(at) >= 8, len(at)
    recipe = [(int(order[j]), 2 + i % 2, [(int(order[j]), 1, 0.75), (int(order[j + 1]), 1, 0.75)], 20) for i, j in enumerate(at)]
    batch = crafted(host, recipe, seed=13)
    params = ScorerParams(min_matched_peaks=min_matched_peaks, report_psms=report_psms, precursor_tol=Tolerance("da", -20.0, 20.0))
    routes = check(w, batch, params, monkeypatch, f"two heavy, report_psms={report_psms}, min_matched_peaks={min_matched_peaks}", default_flags=True)
    assert routes[0] > len(recipe), routes  # (more heavy chunks on the route than spectra: some spectrum had two)
    check(w, batch, params, monkeypatch, f"two heavy, every candidate, report_psms={report_psms}, min_matched_peaks={min_matched_peaks}")


@pytest.mark.parametrize("report_psms", [1, 5])
def test_the_synthetic_world(worlds, monkeypatch, report_psms):
    """the C3-like world (charges 2 / 3 / 4: an ion matched at two charges) and the twin world (ties at the top: the replay)"""
    for name in ("narrow", "ties"):
        w = worlds[name]
        kw = dict(precursor_tol=Tolerance("da", -20.0, 20.0)) if name == "ties" else {}
        check(w, w.batch, ScorerParams(report_psms=report_psms, **kw), monkeypatch, f"{name}, report_psms={report_psms}")


def test_general_instance_and_chimera_rounds_keep_the_trip_per_charge(worlds, monkeypatch):
    w = worlds["narrow"]
    check(w, w.batch, ScorerParams(report_psms=2), monkeypatch, "narrow, general instance", general=True, one_trip=False, fallbacks=True)
    check(w, w.batch, ScorerParams(chimera=True, report_psms=3), monkeypatch, "narrow, chimera", one_trip=False, fallbacks=True)


def test_fragment_charges(worlds, high_charge_world, monkeypatch):
    """precursor charge 4: three fragment charges on the route; 5 and 6: four and five, never on the cooperative path at all"""
    w = high_charge_world
    z = np.asarray(w.batch.precursor_charge)
    assert {4, 5, 6} <= set(z.tolist())
    params = ScorerParams(max_precursor_charge=6, max_fragment_charge=None)
    check(w, w.batch.subset(np.flatnonzero(z == 4)), params, monkeypatch, "charge 4")
    check(w, w.batch.subset(np.flatnonzero(z >= 5)), params, monkeypatch, "charges 5 and 6", one_trip=False, fallbacks=False)
    check(w, w.batch, params, monkeypatch, "charges 4 to 6")
