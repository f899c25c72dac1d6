"""The first precursor window from the schedule record (kernels.hip: window_max_kernel writes {left, right, first, end} of every
spectrum's first query into the third uint4 of a resident batch's records; prelim_spectrum takes it from there instead of searching)
against the same kernels searching as before (SAGE_HIP_DEBUG_FLAGS=65536, read when the scorer is created) and against the oracle:
the same records, counts and preliminary lists, byte for byte.

What the window hangs on — the index, the precursor tolerance, wide_window, the isotope-error and charge ranges — is the uploading
scorer's; a batch scored by a scorer that differs in any of them must not use it (capi.hip: WindowKey)."""
import ctypes as C

import numpy as np
import pytest

from parity_utils import assert_features_equal
from sage_amd import _lib as L
from sage_amd.api import DatabaseParameters, Scorer, ScorerParams, SpectrumBatch, Tolerance
from sage_amd.synthetic import synthetic_fasta
from test_gpu_parity import World

pytestmark = pytest.mark.gpu

NO_RECORD_WINDOWS = 65536  # SAGE_HIP_DEBUG_FLAGS: prelim_spectrum searches although the record holds the window
ENV = ("SAGE_HIP_DEBUG_FLAGS", "SAGE_HIP_XCD_CHUNK", "SAGE_HIP_SCHED_DESC", "SAGE_HIP_WAYS", "SAGE_HIP_WCAP", "SAGE_HIP_NO_SCHED",
       "SAGE_HIP_PHASE_CLOCKS", "SAGE_HIP_NARROW")


@pytest.fixture(scope="module")
def world(gpu_required):
    # C3-like: known charges, +-10 ppm, windows of a handful of candidates
    return World(synthetic_fasta(300, seed=11),
                 DatabaseParameters(bucket_size=2048, enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                                    static_mods={"C": 57.0215}, variable_mods={"M": [15.9949]}), {}, 600, seed=21)


def valid_bytes(f, c):
    return f[np.arange(f.shape[1])[None, :] < c[:, None]].tobytes()


def run(world, batch, params, monkeypatch, flags=0, env=None, hits=True, upload_params=None, clocks=False):
    """One route: scorer (variables read at its creation and at the upload), upload, initial_hits, score_resident.
    upload_params: the batch is uploaded by ANOTHER scorer with these parameters and scored by this one."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if flags:
        monkeypatch.setenv("SAGE_HIP_DEBUG_FLAGS", str(flags))
    if clocks:
        monkeypatch.setenv("SAGE_HIP_PHASE_CLOCKS", "1")
    scorer = Scorer(world.dev, params)
    uploader = Scorer(world.dev, upload_params) if upload_params is not None else scorer
    dbatch = uploader.upload(batch)
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    lists = scorer.initial_hits(dbatch) if hits else None
    gf, gc = scorer.score_resident(dbatch)
    out = dict(f=gf.copy(), c=gc.copy(), lists=lists, timing=scorer.last_timing())
    if clocks:
        cyc = np.zeros(32, np.uint64)
        L.check(L.load().sage_hip_debug_phase_cycles(scorer._h, L.as_ptr(cyc, C.c_uint64)))
        out["cycles"] = cyc
    dbatch.close()
    if uploader is not scorer:
        uploader.close()
    scorer.close()
    return out


def assert_same(a, b, ctx):
    assert np.array_equal(a["c"], b["c"]), f"{ctx}: PSM counts differ"
    assert valid_bytes(a["f"], a["c"]) == valid_bytes(b["f"], b["c"]), f"{ctx}: records differ"
    if a["lists"] is not None and b["lists"] is not None:
        (pa, la, ma, sa), (pb, lb, mb, sb) = a["lists"], b["lists"]
        assert np.array_equal(la, lb) and np.array_equal(ma, mb) and np.array_equal(sa, sb), f"{ctx}: list lengths / matched_peaks / scored_candidates differ"
        keep = np.arange(pa.shape[1])[None, :] < la[:, None]
        assert pa[keep].tobytes() == pb[keep].tobytes(), f"{ctx}: preliminary lists differ"


def check(world, batch, params, monkeypatch, ctx, env=None, hits=True, want_psms=True):
    """record windows / searched windows: equal to each other and to the oracle.  Returns (PSMs, the default route's run)."""
    with_w = run(world, batch, params, monkeypatch, 0, env, hits)
    without = run(world, batch, params, monkeypatch, NO_RECORD_WINDOWS, env, hits)
    assert_same(with_w, without, ctx)
    of, oc, _, _ = world.orc.score(params, batch)
    n = assert_features_equal(with_w["f"], with_w["c"], of, oc, ctx + " (record windows)")
    assert assert_features_equal(without["f"], without["c"], of, oc, ctx + " (searched)") == n
    assert (n > 0) == want_psms, ctx
    return n, with_w


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


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65])
def test_small_batches(world, monkeypatch, n):
    check(world, world.batch.subset(np.arange(n)), ScorerParams(), monkeypatch, f"n={n}")


@pytest.mark.parametrize("desc", ["0", "1"])
@pytest.mark.parametrize("n", [8 * 5 * 3 - 1, 8 * 5 * 3 + 1])
def test_across_the_xcd_chunks_in_both_schedule_orders(world, monkeypatch, n, desc):
    """chunks of 5 schedule positions per XCD: the batch ends one short of / one beyond a round of 8 chunks; ascending and descending"""
    check(world, world.batch.subset(np.arange(n)), ScorerParams(), monkeypatch, f"n={n}, desc={desc}",
          env={"SAGE_HIP_XCD_CHUNK": "5", "SAGE_HIP_SCHED_DESC": desc})


def test_step_in_two_parts_steps_through_the_records_by_their_stride(world, monkeypatch):
    """SAGE_HIP_WAYS=2 needs 16 384 spectra: the second part starts at record n / 2 — three uint4 each, not two"""
    idx = np.arange(16400) % world.batch.n
    batch = world.batch.subset(idx)
    params = ScorerParams()
    n, two = check(world, batch, params, monkeypatch, "two parts", env={"SAGE_HIP_WAYS": "2"}, hits=False)
    one = run(world, batch, params, monkeypatch, 0, {"SAGE_HIP_WAYS": "1"}, hits=False)
    assert_same(two, one, "two parts against one")
    # every copy of a spectrum gets its own spectrum's answer, wherever the schedule put it
    base = run(world, world.batch, params, monkeypatch, 0, None, hits=False)
    assert np.array_equal(two["c"], base["c"][idx])
    assert np.array_equal(two["f"]["peptide_idx"][:, 0][two["c"] > 0], base["f"]["peptide_idx"][:, 0][idx][two["c"] > 0])
    assert n > 8000


def test_without_schedule_records(world, monkeypatch):
    check(world, world.batch, ScorerParams(), monkeypatch, "SAGE_HIP_NO_SCHED=1", env={"SAGE_HIP_NO_SCHED": "1"})


@pytest.mark.parametrize("variant", ["probe", "stream"])
def test_peak_counts_charges_and_isotope_errors(world, monkeypatch, variant):
    env = {"SAGE_HIP_NARROW": variant}
    rng = np.random.default_rng(7)
    counts = [0, 1, 192, 193, 300, 64, 65, 128, 191, 2, 300, 0, 150, 193]  # (300: the batch's pcap)
    odd = with_peaks(world.batch, rng, counts)
    assert int(np.diff(odd.peak_off.astype(np.int64)).max()) == 300
    check(world, odd, ScorerParams(min_matched_peaks=2), monkeypatch, f"{variant}: peak counts", env=env)
    check(world, odd, ScorerParams(min_matched_peaks=2, precursor_tol=Tolerance("da", -1.5, 1.5), report_psms=3), monkeypatch,
          f"{variant}: peak counts, +-1.5 Da", env=env)
    b = world.batch
    unknown = SpectrumBatch(b.peak_off, b.masses, b.intensities, b.precursor_mz, np.zeros(b.n, np.uint8), b.total_ion_current)
    # (several queries per spectrum: only the first — the lowest charge, the first isotope error — comes from the record)
    check(world, unknown, ScorerParams(precursor_tol=Tolerance("da", -0.5, 0.5)), monkeypatch, f"{variant}: charge None", env=env)
    check(world, b, ScorerParams(min_isotope_err=-1, max_isotope_err=3, precursor_tol=Tolerance("ppm", -20.0, 20.0)), monkeypatch,
          f"{variant}: isotope errors -1..3", env=env)
    check(world, unknown, ScorerParams(min_isotope_err=-1, max_isotope_err=2, precursor_tol=Tolerance("ppm", -20.0, 20.0)), monkeypatch,
          f"{variant}: isotope errors, charge None", env=env)


def test_isolation_windows_of_a_wide_window_search(world, monkeypatch):
    b = world.batch
    rng = np.random.default_rng(11)
    lo = -rng.uniform(0.3, 1.2, b.n).astype(np.float32)
    hi = rng.uniform(0.3, 1.2, b.n).astype(np.float32)
    lo[::7] = np.nan  # (no isolation window recorded: the +-2.4 default)
    windows = SpectrumBatch(b.peak_off, b.masses, b.intensities, b.precursor_mz, b.precursor_charge, b.total_ion_current, lo, hi)
    check(world, windows, ScorerParams(wide_window=True, chimera=True, report_psms=2), monkeypatch, "wide window")


def test_narrow_spectra_mixed_with_windows_beyond_the_lds_counters(world, monkeypatch):
    """a capacity of 64 slots and +-2 Da: the record's window says `potential > wcap` for part of the batch — those spectra go to the
    large-window kernels, the others stay; each spectrum is scored once, by its own window"""
    params = ScorerParams(precursor_tol=Tolerance("da", -2.0, 2.0))
    sub = world.batch.subset(np.arange(0, world.batch.n, 3))
    n, r = check(world, sub, params, monkeypatch, "mixed", env={"SAGE_HIP_WCAP": "64"})
    wide = r["timing"]["n_wide"]
    print(f"{wide} of {sub.n} spectra handed to the large-window kernels")
    assert 0 < wide < sub.n
    assert n > 100


def test_a_batch_scored_by_a_scorer_its_windows_do_not_belong_to(world, monkeypatch):
    """uploaded by a +-10 ppm scorer, scored by others: the result is that of the scoring scorer's own upload"""
    base = ScorerParams()
    assert base.precursor_tol.kind == "ppm" and abs(base.precursor_tol.hi - 10.0) < 1e-6
    b = world.batch
    unknown = SpectrumBatch(b.peak_off, b.masses, b.intensities, b.precursor_mz, np.zeros(b.n, np.uint8), b.total_ion_current)
    differ = 0
    for name, batch, other in (("+-50 ppm", b, ScorerParams(precursor_tol=Tolerance("ppm", -50.0, 50.0))),
                               ("+-1 Da", b, ScorerParams(precursor_tol=Tolerance("da", -1.0, 1.0))),
                               ("one-sided", b, ScorerParams(precursor_tol=Tolerance("ppm", -10.0, 30.0))),
                               ("isotope errors", b, ScorerParams(min_isotope_err=-1, max_isotope_err=1)),
                               ("charge range", unknown, ScorerParams(min_precursor_charge=3, max_precursor_charge=4))):
        own = run(world, batch, other, monkeypatch)
        foreign = run(world, batch, other, monkeypatch, upload_params=base)
        assert_same(foreign, own, f"fingerprint, {name}")
        of, oc, _, _ = world.orc.score(other, batch)
        assert_features_equal(foreign["f"], foreign["c"], of, oc, f"fingerprint, {name}")
        narrow = run(world, batch, base, monkeypatch)
        differ += not (np.array_equal(narrow["c"], own["c"]) and valid_bytes(narrow["f"], narrow["c"]) == valid_bytes(own["f"], own["c"]))
    assert differ >= 3  # (the other scorers' answers are not the uploading scorer's: stale windows would show)
    # ... and a second scorer with the SAME parameters (a clone in all but name) uses them: same records
    same = run(world, b, ScorerParams(), monkeypatch, upload_params=ScorerParams())
    assert_same(same, run(world, b, ScorerParams(), monkeypatch), "same parameters, another handle")


def test_phase_clocks_with_and_without_record_windows(world, monkeypatch):
    """the profiling instance: the same records, and clock slots that are deltas of ascending marks (a slot that went backwards would
    show as a wrapped 64-bit sum); with the window in the record the search slot holds later queries only — here there are none"""
    params = ScorerParams()
    rec = run(world, world.batch, params, monkeypatch, 0, {"SAGE_HIP_NARROW": "probe"}, hits=False, clocks=True)
    srch = run(world, world.batch, params, monkeypatch, NO_RECORD_WINDOWS, {"SAGE_HIP_NARROW": "probe"}, hits=False, clocks=True)
    assert_same(rec, srch, "profiling instance")
    for name, r in (("record", rec), ("searched", srch)):
        slots = r["cycles"][:5].astype(np.float64) / world.batch.n
        print(name, "cycles per spectrum: staging %d search %d match %d trim %d output %d" % tuple(slots))
        assert np.all(r["cycles"][:5] > 0) and np.all(slots < 5e6), (name, slots)
    assert int(rec["cycles"][7]) == int(srch["cycles"][7]) >= world.batch.n  # the same queries either way (one per spectrum and retry)
