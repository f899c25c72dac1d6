"""The cooperative path of score_candidates (kernels.hip: a candidate with many hits in a 64-ion chunk is matched by the whole
wavefront) takes the candidate's matched counts and longest runs from its hit ballots — core.h: kind_seg_first / kind_seg_next,
run_matched_mask — and adds only the intensities and ppm terms item by item.  The independent route is the dense list / the walk,
which keep the sequential run_matched_packed: SAGE_HIP_DEBUG_FLAGS=32 sends every candidate there.  Per case the records under

    0                   the default choice (more than COOP_MIN_HITS hits, at most COOP_MAX_LANES such candidates)
    32                  no cooperative path
    64                  every such candidate
    64 | 32768          every candidate from its first hit: the whole world goes through the mask forms
    64 | 32768 | 128    ... and whoever is left takes the walk instead of the dense list

are equal byte for byte, and equal to the oracle.  The cases are the smallest shapes at which the segments and the runs can go wrong:
peptides of 2, 5, 33, 34 and 70 residues (one-bit segments; a segment seam at bit 32 of a full chunk; a y segment and a run across
the chunk seam; three chunks), six ion kinds (consecutive segments of one series), precursor charges 2 to 6 (an ion matched at
several fragment charges; four and five fragment charges, which never take the path), min_matched_peaks 1 and 4, report_psms 1
and 5, chimera rounds and SAGE_HIP_RESCORE_GENERAL=1 (the general instance), the isoleucine / leucine twin world (the tie replay,
narrow_kernel), lists wider than a wavefront (rescore_big_kernel) and peptides beyond 1023 residues (its two-register runs).

The cases cannot pass vacuously: the profiling instance's counters (SAGE_HIP_PHASE_CLOCKS=1, sage_hip_debug_heavy_counters) must
show chunks and items on the path under 64 | 32768 and none under 32.  A LIMIT of that proof: rescore_big_kernel (lists wider than a
wavefront, peptides beyond 1023 residues) is compiled without a profiling instance and counts nothing, so its two cases only hold
the five settings and the oracle equal — that the two-register run_matched_mask ran there follows from the code (score_candidates is
shared and reads the flags itself), not from a counter; on the host the wide form is held to the sequential one by
tests/test_run_mask_emulation.py."""
import ctypes as C

import numpy as np
import pytest

from parity_utils import assert_features_equal
from sage_amd import _lib as L
from sage_amd.api import DatabaseParameters, RawSpectrum, Scorer, ScorerParams, SpectrumBatch, SpectrumProcessor, Tolerance
from sage_amd.synthetic import synthetic_fasta
from test_gpu_parity import World

pytestmark = pytest.mark.gpu

NO_COOP, EVERY_HEAVY, WALK, FIRST_HIT = 32, 64, 128, 32768
FLAG_SETS = (0, NO_COOP, EVERY_HEAVY, EVERY_HEAVY | FIRST_HIT, EVERY_HEAVY | FIRST_HIT | WALK)
ENZYME = dict(missed_cleavages=1, cleave_at="KR", restrict="P")
ENV = ("SAGE_HIP_RESCORE_GENERAL", "SAGE_HIP_DEBUG_FLAGS", "SAGE_HIP_PHASE_CLOCKS")


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
    heavy = None
    if clocks:
        out = np.zeros(2, np.uint64)
        L.check(L.load().sage_hip_debug_heavy_counters(scorer._h, L.as_ptr(out, C.c_uint64)))
        heavy = (int(out[0]), int(out[1]))
    scorer.close()
    return gf, gc, heavy


def records(gf, gc):
    return gc.tobytes() + gf[np.arange(gf.shape[1])[None, :] < gc[:, None]].tobytes()


def check(world, batch, params, monkeypatch, ctx, general=False, path=True):
    """the five settings against each other and against the oracle; then the profiling instance: on the path under 64 | 32768 (where
    `path` says some candidate can take it; None: rescore_big_kernel, which has no profiling instance and counts nothing), never
    under 32.  Returns the (chunks, items) of the forced path."""
    of, oc = world.orc.score(params, batch)[:2]
    base = None
    for flags in FLAG_SETS:
        gf, gc, _ = run(world, batch, params, monkeypatch, flags, general)
        n = assert_features_equal(gf, gc, of, oc, f"{ctx}, flags={flags}, general={general}")
        if base is None:
            base = records(gf, gc)
            assert n > 0, ctx
        assert records(gf, gc) == base, f"{ctx}, general={general}: flags={flags} changed the records"
    gf, gc, forced = run(world, batch, params, monkeypatch, EVERY_HEAVY | FIRST_HIT, general, clocks=True)
    assert records(gf, gc) == base, f"{ctx}: the profiling instance, every candidate on the path"
    gf, gc, off = run(world, batch, params, monkeypatch, NO_COOP, general, clocks=True)
    assert records(gf, gc) == base, f"{ctx}: the profiling instance, no cooperative path"
    print(f"{ctx}, general={general}: heavy (chunks, items) forced {forced}, switched off {off}")
    assert off == (0, 0), (ctx, off)
    if path is None:
        assert forced == (0, 0), (ctx, forced)
    elif path:
        # (a chunk on the path has at least one bitmap hit; its matches are at most its hits)
        assert forced[0] > 0 and forced[1] > 0, (ctx, forced)
    else:
        assert forced == (0, 0), (ctx, forced)
    return forced


@pytest.fixture(scope="module")
def worlds(gpu_required):
    # C3-like: known charges 2 / 3 / 4 (one to three fragment charges), +-10 ppm, windows of a handful of candidates
    narrow = World(synthetic_fasta(300, seed=11),
                   DatabaseParameters(bucket_size=2048, enzyme=ENZYME, static_mods={"C": 57.0215}, variable_mods={"M": [15.9949]}),
                   {}, 300, seed=21)
    # tie-rich: every peptide beside its isoleucine / leucine twin (equal masses and fragments: equal hyperscores at the top)
    fasta = synthetic_fasta(60, seed=17)
    twin = fasta.replace("I", "#").replace("L", "I").replace("#", "L").replace(">sp|SYN", ">sp|TWN")
    ties = World(fasta + twin, DatabaseParameters(bucket_size=1024, enzyme=ENZYME, static_mods={"C": 57.0215}), {}, 200, seed=29)
    return dict(narrow=narrow, ties=ties)


def length_world(ion_kinds):
    # peptides of 2 .. 70 residues: 2, 8, 64 and 66 ions with two kinds (2, 5, 33 and 34 residues) and three chunks (70)
    return World(synthetic_fasta(120, seed=41),
                 DatabaseParameters(bucket_size=1024, enzyme=dict(missed_cleavages=2, min_len=2, max_len=70, cleave_at="KR", restrict="P"),
                                    peptide_min_mass=150.0, peptide_max_mass=9000.0, static_mods={"C": 57.0215}, ion_kinds=ion_kinds),
                 {}, 240, seed=43)


@pytest.fixture(scope="module")
def length_worlds(gpu_required):
    return {"by": length_world(["b", "y"]), "abcxyz": length_world(["a", "b", "c", "x", "y", "z"])}


@pytest.fixture(scope="module")
def high_charge_world(gpu_required):
    # precursor charges 4, 5 and 6 with max_fragment_charge None: three (filtered), four and five (unfiltered) fragment charges
    return World(synthetic_fasta(150, seed=47),
                 DatabaseParameters(bucket_size=1024, enzyme=dict(missed_cleavages=2, cleave_at="KR", restrict="P"), static_mods={"C": 57.0215}),
                 dict(charges=((4, 0.4), (5, 0.3), (6, 0.3))), 160, seed=53)


@pytest.mark.parametrize("min_matched_peaks", [1, 4])
@pytest.mark.parametrize("kinds", ["by", "abcxyz"])
def test_peptide_lengths_and_ion_kinds(length_worlds, monkeypatch, kinds, min_matched_peaks):
    """2, 5, 33, 34 and 70 residues x two and six ion kinds x the prune's bound 1 (a lone match passes: a 2-residue peptide's single
    b ion, index 0, counts and makes no run) and 4"""
    w = length_worlds[kinds]
    lens = set(np.diff(w.host.seq_off.astype(np.int64)).tolist())
    assert {2, 5, 33, 34, 70} <= lens, sorted(lens)
    check(w, w.batch, ScorerParams(min_matched_peaks=min_matched_peaks), monkeypatch, f"lengths, {kinds}, min_matched_peaks={min_matched_peaks}")


@pytest.mark.parametrize("kinds", ["by", "abcxyz"])
def test_short_beside_long_in_one_list(length_worlds, monkeypatch, kinds):
    """+-300 Da, five PSMs: candidates of one, two and three chunks in one list, min_matched_peaks 1"""
    w = length_worlds[kinds]
    sub = w.batch.subset(np.arange(0, w.batch.n, 2))
    check(w, sub, ScorerParams(min_matched_peaks=1, report_psms=5, precursor_tol=Tolerance("da", -300.0, 300.0)), monkeypatch,
          f"lengths, {kinds}, +-300 Da")


@pytest.mark.parametrize("report_psms", [1, 5])
@pytest.mark.parametrize("name", ["narrow", "ties"])
def test_both_instances(worlds, monkeypatch, name, report_psms):
    """the C3-like world and the twin world x report_psms 1 and 5, the instance without chimera rounds and the general one"""
    w = worlds[name]
    kw = dict(precursor_tol=Tolerance("da", -20.0, 20.0)) if name == "ties" else {}
    for general in (False, True):
        check(w, w.batch, ScorerParams(report_psms=report_psms, **kw), monkeypatch, f"{name}, report_psms={report_psms}", general=general)


def test_chimera_rounds(worlds, monkeypatch):
    """the general instance: a second round against the spectrum without the winner's peaks"""
    w = worlds["narrow"]
    check(w, w.batch, ScorerParams(chimera=True, report_psms=3), monkeypatch, "narrow, chimera")
    t = worlds["ties"]
    check(t, t.batch, ScorerParams(chimera=True, report_psms=2, precursor_tol=Tolerance("da", -20.0, 20.0)), monkeypatch, "ties, chimera")


def test_fragment_charges(worlds, high_charge_world, monkeypatch):
    """precursor charges 2, 3, 4 (one to three fragment charges, an ion matched at several of them) are in the C3-like world; here 4,
    5 and 6: three fragment charges on the path, four and five never on it — alone, and beside the others in one list"""
    assert {2, 3, 4} <= set(np.asarray(worlds["narrow"].batch.precursor_charge).tolist())
    w = high_charge_world
    z = np.asarray(w.batch.precursor_charge)
    assert {4, 5, 6} <= set(z.tolist())
    check(w, w.batch, ScorerParams(max_precursor_charge=6, max_fragment_charge=None), monkeypatch, "charges 4 to 6")
    check(w, w.batch.subset(np.flatnonzero(z >= 5)), ScorerParams(max_precursor_charge=6, max_fragment_charge=None), monkeypatch,
          "charges 5 and 6: four and five fragment charges", path=False)
    mixed = ScorerParams(max_precursor_charge=6, override_precursor_charge=True, max_fragment_charge=None, report_psms=3,
                         precursor_tol=Tolerance("da", -3.0, 3.0))
    check(w, w.batch.subset(np.arange(0, w.batch.n, 2)), mixed, monkeypatch, "charges 2 to 6 in one list")


def test_lists_wider_than_a_wavefront(worlds, monkeypatch):
    """report_psms > 32: rescore_big_kernel's one-register instance"""
    w = worlds["narrow"]
    sub = w.batch.subset(np.arange(0, w.batch.n, 3))
    check(w, sub, ScorerParams(report_psms=40, precursor_tol=Tolerance("da", -60.0, 60.0)), monkeypatch, "report_psms=40", path=None)


def test_peptides_beyond_1023_residues(gpu_required, monkeypatch):
    """rescore_big_kernel's LONG instance: the two-register runs, ladders of consecutive b / y ions far beyond index 1023 — runs of
    dozens of ions across many chunk seams, the y series' segment starting inside a chunk"""
    from sage_amd.synthetic import _MASS_LUT, PROTON
    rng = np.random.default_rng(191)
    letters = list("ADEFGHILMNQSTVWY")  # no K / R: trypsin finds nothing to cut
    fasta = "".join(f">sp|LONG{i}|LONG{i}\n{''.join(rng.choice(letters, n))}\n" for i, n in enumerate((1100, 1301, 1024, 1023)))
    dbp = DatabaseParameters(bucket_size=1024, enzyme=dict(missed_cleavages=0, min_len=1000, max_len=3000, cleave_at="KR", restrict="P"),
                             peptide_min_mass=500.0, peptide_max_mass=400000.0, static_mods={"C": 57.0215})
    w = World(fasta, dbp, {}, 4, seed=3)  # (the world's own synthetic spectra stop at 2 500 Th: replaced below)
    host = w.host
    seq_off = host.seq_off.astype(np.int64)
    spectra = []
    for i in range(12):
        pep = int(np.flatnonzero(host.decoy == 0)[i % 4])
        a, b = seq_off[pep], seq_off[pep + 1]
        res = _MASS_LUT[host.seq[a:b]] + host.mods[a:b].astype(np.float64)
        mono = float(host.pep_mono[pep])
        z = int(rng.choice([2, 3, 4]))
        bs = np.cumsum(res)[:-1]
        ys = mono - bs
        n_ions = len(bs)
        lo = int(rng.integers(n_ions // 2, n_ions - 120))
        lad = np.arange(lo, lo + int(rng.integers(60, 110)))
        lad = lad[rng.random(len(lad)) < 0.9]  # (with gaps: several runs, one of them the longest)
        mz = np.concatenate([bs[lad] + PROTON, ys[lad[: len(lad) // 3]] + PROTON, (bs[lad[::5]] + 2 * PROTON) / 2.0, rng.uniform(150.0, mono, 60)])
        mz = mz * (1.0 + rng.normal(0.0, 2.0, len(mz)) * 1e-6)
        it = np.concatenate([rng.lognormal(9.0, 0.5, len(mz) - 60), rng.lognormal(6.0, 1.0, 60)])
        order = np.argsort(mz, kind="stable")
        spectra.append(RawSpectrum(mz[order].astype(np.float32), it[order].astype(np.float32), float(np.float32((mono + z * PROTON) / z)), z, None,
                                   scan_start_time=float(i), file_id=0, id=f"scan={i}"))
    batch = SpectrumBatch.from_spectra([SpectrumProcessor(150, False, 0.0).process(r) for r in spectra])
    params = ScorerParams(precursor_tol=Tolerance("da", -200000.0, 200000.0), fragment_tol=Tolerance("ppm", -20.0, 20.0), report_psms=3)
    check(w, batch, params, monkeypatch, "peptides beyond 1023 residues", path=None)
    gf, gc, _ = run(w, batch, params, monkeypatch, EVERY_HEAVY | FIRST_HIT)
    assert int(gc.min()) >= 1 and int(gf[np.arange(batch.n), 0]["longest_b"].max()) > 20
