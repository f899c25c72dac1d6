"""The hand-over of the narrow first pass in schedule order (device_types.h: DevWork::hand — prelim_kernel leaves a spectrum's
preliminary list, status, length and totals in ONE 512-byte row at its schedule position, rescore_kernel reads the row beside the
schedule record instead of behind it) against the same kernels handing over in the arrays indexed by spectrum
(SAGE_HIP_DEBUG_FLAGS=131072, read when the scorer is created) and against the oracle: the same records, counts and preliminary
lists, byte for byte.  sage_hip_debug_handover_route says which route the last step took: the cases that must take the rows
assert that they did, and those that must keep the arrays — report_psms 32, large windows in the step, no schedule records — that
they did not."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from parity_utils import assert_features_equal
from sage_amd import _lib as L
from sage_amd.api import DatabaseParameters, Scorer, ScorerParams, SpectrumBatch, Tolerance
from sage_amd.synthetic import synthetic_fasta
from test_gpu_parity import World

pytestmark = pytest.mark.gpu

BY_SPECTRUM = 131072  # SAGE_HIP_DEBUG_FLAGS: the hand-over arrays indexed by spectrum, whatever the step
ENV = ("SAGE_HIP_DEBUG_FLAGS", "SAGE_HIP_XCD_CHUNK", "SAGE_HIP_SCHED_DESC", "SAGE_HIP_WAYS", "SAGE_HIP_WCAP", "SAGE_HIP_NO_SCHED",
       "SAGE_HIP_ASSUME_NARROW", "SAGE_HIP_NO_FAST_TIES", "SAGE_HIP_CHUNK")
NO_CANDIDATE = np.uint64(0x0000FFFFFFFF0080)  # core.h: PRESCORE_EMPTY, the packed default PreScore (no peptide)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# windows of a few hundred candidates (at most 550 of the 1024 slots prelim_kernel counts in, so the upload still says "no large
# windows"): the trims drop candidates and the lists are full
WIDER = Tolerance("da", -8.0, 8.0)
TWINS_WIDER = Tolerance("da", -20.0, 20.0)  # (the twins' index is a fifth of the size: windows of up to 376 candidates)


def make_world():
    # C3-like: known charges, +-10 ppm, windows of a handful of candidates
    return World(synthetic_fasta(300, seed=11),
                 DatabaseParameters(bucket_size=2048, enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                                    static_mods={"C": 57.0215}, variable_mods={"M": [15.9949]}), {}, 600, seed=21)


@pytest.fixture(scope="module")
def world(gpu_required):
    return make_world()


@pytest.fixture(scope="module")
def twins(gpu_required):
    """isoleucine / leucine twins (identical masses and fragments): equal hyperscores at the top of most spectra"""
    fasta = synthetic_fasta(60, seed=17)
    twin = fasta.replace("I", "#").replace("L", "I").replace("#", "L").replace(">sp|SYN", ">sp|TWN")
    return World(fasta + twin, DatabaseParameters(bucket_size=1024, enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                                                  static_mods={"C": 57.0215}), {}, 300, seed=29)


def valid_bytes(f, c):
    return f[np.arange(f.shape[1])[None, :] < c[:, None]].tobytes()


def route_of(scorer):
    out = np.zeros(1, np.uint32)
    L.check(L.load().sage_hip_debug_handover_route(scorer._h, L.as_ptr(out, C.c_uint32)))
    return int(out[0])


def run(world, batch, params, monkeypatch, flags=0, env=None, hits=True, upload_params=None, stream=False, clone=False):
    """One route: scorer (variables read at its creation and at the upload), upload, initial_hits, score_resident.
    upload_params: the batch is uploaded by ANOTHER scorer with these parameters and scored by this one.
    stream: Scorer.score, the upload / score / download pipeline, instead.  clone: a clone of the scorer does the scoring."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if flags:
        monkeypatch.setenv("SAGE_HIP_DEBUG_FLAGS", str(flags))
    first = Scorer(world.dev, params)
    scorer = first.clone() if clone else first
    if stream:
        gf, gc = scorer.score(batch)
        out = dict(f=gf.copy(), c=gc.copy(), lists=None, timing=scorer.last_timing(), route=route_of(scorer))
        for var in ENV:
            monkeypatch.delenv(var, raising=False)
    else:
        uploader = Scorer(world.dev, upload_params) if upload_params is not None else scorer
        dbatch = uploader.upload(batch)
        for var in ENV:
            monkeypatch.delenv(var, raising=False)
        lists = scorer.initial_hits(dbatch) if hits else None
        gf, gc = scorer.score_resident(dbatch)
        out = dict(f=gf.copy(), c=gc.copy(), lists=lists, timing=scorer.last_timing(), route=route_of(scorer))
        dbatch.close()
        if uploader is not scorer:
            uploader.close()
    if scorer is not first:
        scorer.close()
    first.close()
    return out


def assert_same(a, b, ctx):
    assert np.array_equal(a["c"], b["c"]), f"{ctx}: PSM counts differ"
    assert valid_bytes(a["f"], a["c"]) == valid_bytes(b["f"], b["c"]), f"{ctx}: records differ"
    if a["lists"] is not None and b["lists"] is not None:
        (pa, la, ma, sa), (pb, lb, mb, sb) = a["lists"], b["lists"]
        assert np.array_equal(la, lb) and np.array_equal(ma, mb) and np.array_equal(sa, sb), f"{ctx}: list lengths / matched_peaks / scored_candidates differ"
        keep = np.arange(pa.shape[1])[None, :] < la[:, None]
        assert pa[keep].tobytes() == pb[keep].tobytes(), f"{ctx}: preliminary lists differ"


def check(world, batch, params, monkeypatch, ctx, env=None, hits=True, want_psms=True, rows=True, oracle=None, **how):
    """rows / arrays by spectrum: equal to each other and to the oracle; the default route is the rows where `rows` says so, the
    flag's never.  Returns (PSMs, the default route's run)."""
    by_row = run(world, batch, params, monkeypatch, 0, env, hits, **how)
    by_spec = run(world, batch, params, monkeypatch, BY_SPECTRUM, env, hits, **how)
    assert by_row["route"] == (1 if rows else 0), f"{ctx}: the default route handed over {'by spectrum' if rows else 'in rows'}"
    assert by_spec["route"] == 0, f"{ctx}: SAGE_HIP_DEBUG_FLAGS={BY_SPECTRUM} handed over in rows"
    assert_same(by_row, by_spec, ctx)
    of, oc = oracle if oracle is not None else world.orc.score(params, batch)[:2]
    n = assert_features_equal(by_row["f"], by_row["c"], of, oc, ctx + " (default route)")
    assert assert_features_equal(by_spec["f"], by_spec["c"], of, oc, ctx + " (by spectrum)") == n
    assert (n > 0) == want_psms, ctx
    return n, by_row


def with_peaks(batch, rng, counts):
    """the batch's first len(counts) spectra with exactly counts[i] peaks each: their own, cut or filled up with noise, ascending"""
    off, masses, ints = [0], [], []
    for i, want in enumerate(counts):
        a, e = int(batch.peak_off[i]), int(batch.peak_off[i + 1])
        m, it = batch.masses[a:e][:want], batch.intensities[a:e][:want]
        if len(m) < want:
            extra = rng.uniform(150.0, 1800.0, want - len(m)).astype(np.float32)
            m = np.concatenate([m, extra])
            it = np.concatenate([it, rng.uniform(1.0, 50.0, len(extra)).astype(np.float32)])
            order = np.argsort(m, kind="stable")
            m, it = m[order], it[order]
        masses.append(m)
        ints.append(it)
        off.append(off[-1] + want)
    k = len(counts)
    cat = lambda parts: np.concatenate(parts).astype(np.float32) if off[-1] else np.zeros(0, np.float32)
    tic = np.array([float(np.sum(x)) for x in ints], np.float32)
    return SpectrumBatch(np.array(off, np.uint64), cat(masses), cat(ints), batch.precursor_mz[:k].copy(), batch.precursor_charge[:k].copy(), tic)


def unknown_charges(b):
    return SpectrumBatch(b.peak_off, b.masses, b.intensities, b.precursor_mz, np.zeros(b.n, np.uint8), b.total_ion_current)


# ---- batch shape and schedule order ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65])
def test_small_batches(world, monkeypatch, n):
    check(world, world.batch.subset(np.arange(n)), ScorerParams(), monkeypatch, f"n={n}")


@pytest.mark.parametrize("desc", ["0", "1"])
@pytest.mark.parametrize("n", [8 * 5 * 3 - 1, 8 * 5 * 3 + 1])
def test_across_the_xcd_chunks_in_both_schedule_orders(world, monkeypatch, n, desc):
    """chunks of 5 schedule positions per XCD: the batch ends one short of / one beyond a round of 8 chunks; ascending and descending"""
    check(world, world.batch.subset(np.arange(n)), ScorerParams(), monkeypatch, f"n={n}, desc={desc}",
          env={"SAGE_HIP_XCD_CHUNK": "5", "SAGE_HIP_SCHED_DESC": desc})


@pytest.fixture(scope="module")
def tiled(world):
    """the 600 spectra over and over, 3 x 8192 in all (a step goes in `ways` parts from 8192 spectra per part), and the oracle's answer"""
    batch = world.batch.subset(np.arange(3 * 8192) % world.batch.n)
    return batch, world.orc.score(ScorerParams(), batch)[:2]


@pytest.mark.parametrize("ways", [1, 2, 3])
def test_step_in_parts_each_with_its_own_rows(world, tiled, monkeypatch, ways):
    """part p owns the rows [start_p, start_p + n_p) of the launch's array, as it owns those entries of the count rows and the lists"""
    batch, oracle = tiled
    n, r = check(world, batch, ScorerParams(), monkeypatch, f"{ways} parts", env={"SAGE_HIP_WAYS": str(ways)}, hits=False, oracle=oracle)
    assert r["timing"]["n_ways"] == ways and n > 12000


def grid_child(path):
    """(a process of its own: kernels.hip reads SAGE_HIP_PRELIM_GRID once per process)"""
    w = make_world()
    with pytest.MonkeyPatch.context() as mp:
        by_row = run(w, w.batch, ScorerParams(), mp, 0, None, hits=False)
        by_spec = run(w, w.batch, ScorerParams(), mp, BY_SPECTRUM, None, hits=False)
    assert by_row["route"] == 1 and by_spec["route"] == 0
    assert_same(by_row, by_spec, "capped preliminary grid")
    np.savez(path, f=by_row["f"], c=by_row["c"])


@pytest.mark.parametrize("grid", ["7", "8"])
def test_capped_preliminary_grid(world, monkeypatch, tmp_path, grid):
    """SAGE_HIP_PRELIM_GRID: workgroups of prelim_kernel that stride over the batch — the row is that of the schedule position `blk`,
    not of blockIdx.x.  (The knob keeps multiples of 8 only: 7 caps nothing, 8 is the smallest grid that strides.)"""
    out = tmp_path / "grid.npz"
    env = {k: v for k, v in os.environ.items() if k not in ENV}
    env["SAGE_HIP_PRELIM_GRID"] = grid
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    subprocess.run([sys.executable, "-c", f"import test_gpu_handover_rows as t; t.grid_child({str(out)!r})"], cwd=ROOT, env=env, check=True,
                   timeout=300)
    got = np.load(out)
    of, oc = world.orc.score(ScorerParams(), world.batch)[:2]
    assert assert_features_equal(got["f"], got["c"], of, oc, f"SAGE_HIP_PRELIM_GRID={grid}") > 300


# ---- row and list edge cases -----------------------------------------------------------------------------------------------------
def test_peak_counts_and_an_empty_precursor_window(world, monkeypatch):
    rng = np.random.default_rng(7)
    counts = [0, 1, 192, 193, 300, 64, 65, 128, 191, 2, 300, 0, 150, 193]  # (300: the batch's pcap)
    odd = with_peaks(world.batch, rng, counts)
    assert int(np.diff(odd.peak_off.astype(np.int64)).max()) == 300
    # ... and precursors no peptide of the index is near: the list names no peptide (the reference's list of such a spectrum is not
    # empty: it holds the one default entry of its empty window, which the row carries like any other) and nothing is reported
    odd.precursor_mz[[3, 9]] = np.float32(61.5)
    n, r = check(world, odd, ScorerParams(min_matched_peaks=2), monkeypatch, "peak counts")
    packed, length = r["lists"][:2]
    for i in (3, 9):
        assert length[i] <= 1 and np.all(packed[i, :length[i]] == NO_CANDIDATE)
    assert np.all(r["c"][[0, 3, 9, 11]] == 0)
    check(world, odd, ScorerParams(min_matched_peaks=2, precursor_tol=Tolerance("da", -1.5, 1.5), report_psms=3), monkeypatch,
          "peak counts, +-1.5 Da")


def test_lists_shorter_than_the_trim_and_lists_of_kmax(world, monkeypatch):
    n, r = check(world, world.batch, ScorerParams(report_psms=2), monkeypatch, "+-10 ppm")
    assert int(r["lists"][1].max()) < 50 and r["timing"]["n_retry"] == 0  # no trim dropped anything: ST_OK_ORDERED
    n, r = check(world, world.batch, ScorerParams(report_psms=2, precursor_tol=WIDER), monkeypatch, "+-8 Da")
    assert int(np.sum(r["lists"][1] == 50)) > 100 and r["timing"]["n_wide"] == 0  # lists of exactly kmax


@pytest.mark.parametrize("report_psms", [1, 5, 25, 31, 32])
def test_report_psms_up_to_the_last_list_that_fits_a_row(world, monkeypatch, report_psms):
    """kmax = max(50, 2 * report_psms): 62 words for 31 — the list ends in the lane next to the header — and 64 for 32, which keeps
    the arrays by spectrum"""
    kmax = max(50, 2 * report_psms)
    n, r = check(world, world.batch, ScorerParams(report_psms=report_psms, precursor_tol=WIDER), monkeypatch, f"report_psms={report_psms}",
                 rows=report_psms <= 31)
    assert int(np.sum(r["lists"][1] == kmax)) > 100 and r["timing"]["n_wide"] == 0


def test_chimera_unknown_charges_and_isotope_errors(world, monkeypatch):
    check(world, world.batch, ScorerParams(chimera=True, report_psms=2), monkeypatch, "chimera")  # (the general instance)
    check(world, world.batch, ScorerParams(chimera=True, report_psms=2, precursor_tol=WIDER), monkeypatch, "chimera, +-8 Da")
    unknown = unknown_charges(world.batch)
    # several queries per spectrum
    check(world, unknown, ScorerParams(precursor_tol=Tolerance("da", -0.5, 0.5)), monkeypatch, "charge None")
    check(world, world.batch, ScorerParams(min_isotope_err=-1, max_isotope_err=3, precursor_tol=Tolerance("ppm", -20.0, 20.0)), monkeypatch,
          "isotope errors -1..3")
    check(world, unknown, ScorerParams(min_isotope_err=-1, max_isotope_err=2, precursor_tol=Tolerance("ppm", -20.0, 20.0)), monkeypatch,
          "isotope errors, charge None")


# ---- routes that stay on the arrays by spectrum or survive a repair ------------------------------------------------------------------
def test_wrong_guess_and_mixed_routing(world, monkeypatch):
    """a capacity of 64 slots and +-2 Da: part of the batch has windows beyond the LDS counters.  Told that there are none
    (SAGE_HIP_ASSUME_NARROW=1) the step starts on the rows, prelim_kernel hands those spectra on — rows that say so, and the marks
    by spectrum the host looks for — and the step is repeated with the large-window kernels, on the arrays by spectrum; knowing
    it from the upload, the step takes the arrays at once"""
    params = ScorerParams(precursor_tol=Tolerance("da", -2.0, 2.0))
    sub = world.batch.subset(np.arange(0, world.batch.n, 3))
    for ctx, env in (("wrong guess", {"SAGE_HIP_WCAP": "64", "SAGE_HIP_ASSUME_NARROW": "1"}), ("mixed", {"SAGE_HIP_WCAP": "64"})):
        n, r = check(world, sub, params, monkeypatch, ctx, env=env, rows=False)
        assert 0 < r["timing"]["n_wide"] < sub.n and n > 100


def test_ties_settled_from_the_stored_counts_and_by_the_retry_pass(twins, monkeypatch):
    params = ScorerParams(precursor_tol=TWINS_WIDER)
    n, r = check(twins, twins.batch, params, monkeypatch, "I/L twins, cheap ties")
    assert r["timing"]["n_tied"] > 50 and r["timing"]["n_retry"] <= 2 and r["timing"]["n_wide"] == 0
    n, r = check(twins, twins.batch, params, monkeypatch, "I/L twins, retry pass", env={"SAGE_HIP_NO_FAST_TIES": "1"})
    assert r["timing"]["n_retry"] > 50 and r["timing"]["n_tied"] == 0
    n, r = check(twins, twins.batch, ScorerParams(precursor_tol=TWINS_WIDER, report_psms=2), monkeypatch, "I/L twins, two PSMs")
    assert r["timing"]["n_retry"] > 50


def test_without_schedule_records(world, monkeypatch):
    check(world, world.batch, ScorerParams(), monkeypatch, "SAGE_HIP_NO_SCHED=1", env={"SAGE_HIP_NO_SCHED": "1"}, rows=False)


# ---- reuse and entry points ------------------------------------------------------------------------------------------------------
def test_one_handle_batch_after_batch(world, monkeypatch):
    """600, 65 and 600 spectra on one handle: the rows of the first batch lie under those of the second and are not read for them;
    a larger batch than any before takes a larger array"""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    params = ScorerParams(precursor_tol=WIDER)
    b = world.batch
    rev = b.subset(np.arange(b.n)[::-1].copy())
    batches = [b.subset(np.arange(100, 400)), b, b.subset(np.arange(300, 365)), rev]
    refs = [world.orc.score(params, x)[:2] for x in batches]
    got = {}
    for flags in (0, BY_SPECTRUM):
        if flags:
            monkeypatch.setenv("SAGE_HIP_DEBUG_FLAGS", str(flags))
        scorer = Scorer(world.dev, params)
        monkeypatch.delenv("SAGE_HIP_DEBUG_FLAGS", raising=False)
        for k, (x, (of, oc)) in enumerate(zip(batches, refs)):
            d = scorer.upload(x)
            gf, gc = scorer.score_resident(d)
            assert route_of(scorer) == (0 if flags else 1)
            assert assert_features_equal(gf, gc, of, oc, f"batch {k}, flags {flags}") > x.n // 3
            got[flags, k] = (valid_bytes(gf, gc), gc.copy())
            d.close()
        scorer.close()
    for k in range(len(batches)):
        assert got[0, k][0] == got[BY_SPECTRUM, k][0] and np.array_equal(got[0, k][1], got[BY_SPECTRUM, k][1])


def test_cloned_handle_and_a_batch_of_another_scorer(world, monkeypatch):
    params = ScorerParams(precursor_tol=WIDER)
    n, _ = check(world, world.batch, params, monkeypatch, "clone", clone=True)
    assert n > 300
    # uploaded by a +-10 ppm scorer: its records carry windows that are not this scorer's; the rows do not hang on them
    n, _ = check(world, world.batch, params, monkeypatch, "foreign batch", upload_params=ScorerParams())
    assert n > 300


def test_streaming_entry_in_chunks_on_both_lanes(world, monkeypatch):
    """Scorer.score over chunks of 128 spectra: five chunks through the four input slots and the two compute lanes, each lane with
    a working set — and rows — of its own"""
    for params, ctx in ((ScorerParams(), "narrow"), (ScorerParams(precursor_tol=WIDER, report_psms=3), "+-8 Da")):
        n, r = check(world, world.batch, params, monkeypatch, "pipeline, " + ctx, env={"SAGE_HIP_CHUNK": "128"}, stream=True)
        assert n > 300 and r["timing"]["n_launches"] >= 5 * 2
