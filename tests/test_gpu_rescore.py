"""GPU parity of the post-search rescoring (rescore.hip, through sage_hip_rescore) against the CPU oracle.

The LDA sums (class means, within-class scatter) run strictly in row order on the device, as in the reference; what the product
fixes beyond that is in sage_amd/csrc/detmath.h (IEEE-only ln_1p / exp, blocked order of the kernel-density sums, whose order
the reference leaves to rayon).  Two comparisons per data set:
  * against the oracle in the same mode (`det=True`): every bit that reaches the Gauss-Jordan pivot search is then the same on
    both sides, so the fit-or-heuristic decision, the coefficients, the discriminants, every q-value and the output order are
    held EQUAL — also on data with constant columns (ims == 0 is the normal case without ion mobility), where the elimination
    pivots on rounding noise.  The one exception is log10 of the posterior error (device libm vs glibc): 2 f32 ulps;
  * against the oracle in the reference's own mode (`det=False`: platform libm, every sum sequential): the same
    fit-or-heuristic decision on every data set, and — where no column is constant, i.e. where the coefficients mean
    anything — coefficients to 1e-9, discriminants and posterior errors to 1e-5, spectrum / peptide / protein q-values and the
    output order equal (>= 99.99 % / 99.9 % of the PSMs).  This leg is the INDEPENDENT check: oracle/detmath_oracle.h, which the
    `det=True` leg uses, is a copy of the product's detmath.h (same algorithms, namespace renamed), kept so that the checker does
    not include product headers — equality with it proves the device evaluates the stated contract, not that the contract is right.
"""
import numpy as np
import pytest

import oracle_lib
from rescore_utils import synthetic_features
from sage_amd.api import (DatabaseParameters, DeviceDatabase, Scorer, ScorerParams, SpectrumBatch, SpectrumProcessor, Tolerance,
                          rescore)
from sage_amd.synthetic import synthetic_fasta, synthetic_spectra

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b) or bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def compare(f, tol, pk, npk, prk, npr, context, ref_leg=True, **opt):
    """ref_leg=False leaves out the comparison with the reference-order mode — for inputs on which the oracle's own two modes do
    not meet that leg's thresholds against each other, or on which a second oracle pass costs seconds (test_rescore_edges_cpu.py
    holds every such flag to the data)."""
    g = rescore(f, tol, pk, npk, prk, npr, **opt)
    o = oracle_lib.rescore(f, tol, pk, npk, prk, npr, det=True, **opt)
    n = len(f)
    assert g.lda_fitted == o["lda_fitted"], context
    if g.lda_fitted:
        assert _same(g.coef, o["coef"]), (context, g.coef, o["coef"])  # f64, bit for bit
    assert _same(g.discriminant_score, o["discriminant_score"]), (context, np.flatnonzero(g.discriminant_score != o["discriminant_score"])[:5])
    pe_g, pe_o = g.posterior_error.astype(np.float64), o["posterior_error"].astype(np.float64)
    assert np.all(np.abs(pe_g - pe_o) <= 2.5e-7 * np.maximum(np.abs(pe_o), 1e-30)), (context, np.abs(pe_g - pe_o).max())
    for name, got, exp in (("spectrum_q", g.spectrum_q, o["spectrum_q"]), ("peptide_q", g.peptide_q, o["peptide_q"]),
                           ("protein_q", g.protein_q, o["protein_q"])):
        assert _same(got, exp), (context, name, np.flatnonzero(got != exp)[:5])
    assert np.array_equal(g.order, o["order"]), context
    assert (int(g.passing_spectrum), int(g.passing_peptide), int(g.passing_protein)) == tuple(int(x) for x in o["passing"]), context
    if ref_leg:
        reference_leg(g, oracle_lib.rescore(f, tol, pk, npk, prk, npr, det=False, want_rows=True, **opt), context)
    return g, o


def reference_leg(g, r, context):
    """`g` (the device's result, or anything with its fields) against the reference's own arithmetic (platform libm, sequential
    sums), `r` = oracle_lib.rescore(..., det=False, want_rows=True).  True when the per-PSM half applied (a fitted model, no
    constant column), False when only the fit-or-heuristic decision could be compared."""
    assert g.lda_fitted == r["lda_fitted"], (context, "fit-or-heuristic decision differs from the reference order")
    if g.lda_fitted and all(np.ptp(r["rows"][:, j]) > 0 for j in range(r["rows"].shape[1])):
        scale = np.abs(r["coef"]).max()
        assert np.allclose(g.coef, r["coef"], rtol=1e-9, atol=1e-9 * scale), (context, np.abs(g.coef - r["coef"]).max() / scale)
        assert np.mean(g.spectrum_q == r["spectrum_q"]) > 0.9999, context
        # the per-PSM outputs, too: discriminants and posterior errors (f32 of f64 arithmetic that differs in the last bits between
        # the two libms and summation orders: measured equal on every data set of this file, held to 1e-5), and the q-values of the
        # two picked competitions (equal unless such a last-bit difference swaps two neighbours of the sort)
        assert np.allclose(g.discriminant_score, r["discriminant_score"], rtol=1e-5, atol=1e-6), (context, "discriminant_score vs the reference order")
        assert np.allclose(g.posterior_error, r["posterior_error"], rtol=1e-5, atol=1e-6), (context, "posterior_error vs the reference order")
        for name, got in (("peptide_q", g.peptide_q), ("protein_q", g.protein_q)):
            assert np.mean(got == r[name]) > 0.9999, (context, name, "vs the reference order")
        assert np.mean(g.order == r["order"]) > 0.999, (context, "output order vs the reference order")
        return True
    return False


@pytest.mark.parametrize("n,seed", [(20000, 5), (300, 6), (100000, 8)])
def test_rescore_synthetic_ppm(gpu_required, n, seed):
    f, pk, npk, prk, npr = synthetic_features(n, seed=seed)
    g, o = compare(f, Tolerance("ppm", -10.0, 10.0), pk, npk, prk, npr, f"ppm n={n}")
    assert g.lda_fitted and g.passing_spectrum > 0


def test_rescore_da_tolerance_and_model_inputs(gpu_required):
    """Da precursor tolerance: mass error = expmass - calcmass, 0.1 x bandwidth, max(hi - lo, 1000) bins
    (linear_discriminant.rs:140-157); aligned_rt / delta_rt_model / delta_ims_model arrays as the RT / IM models leave them."""
    f, pk, npk, prk, npr = synthetic_features(30000, seed=9, ppm=False)
    rng = np.random.default_rng(10)
    opt = dict(aligned_rt=rng.uniform(0, 1, len(f)).astype(np.float32),
               delta_rt_model=np.abs(rng.normal(0, 0.05, len(f))).astype(np.float32),
               delta_ims_model=np.abs(rng.normal(0, 0.02, len(f))).astype(np.float32))
    g, _ = compare(f, Tolerance("da", -500.0, 100.0), pk, npk, prk, npr, "da", **opt)
    assert g.lda_fitted


def test_rescore_fallback_paths(gpu_required):
    # no decoys at all: train returns None (linear_discriminant.rs:83-85) -> heuristic discriminant, q = 1 / targets
    f, pk, npk, prk, npr = synthetic_features(5000, seed=11, decoy_frac=0.0)
    g, o = compare(f, Tolerance("ppm", -10.0, 10.0), pk, npk, prk, npr, "no decoys")
    assert not g.lda_fitted and np.all(g.posterior_error == 1.0)
    # constant ims column (the normal case without ion mobility): the elimination meets exact zeros and rounding noise among
    # its pivot candidates; the device must take the oracle's branch whatever it is, on every one of these data sets
    tol = Tolerance("ppm", -10.0, 10.0)
    branches = set()
    for n, seed in ((4000, 3), (900, 14), (12000, 15), (50000, 16), (2500, 17)):
        f, pk, npk, prk, npr = synthetic_features(n, seed=seed, zero_ims=True)
        g, _ = compare(f, tol, pk, npk, prk, npr, f"zero ims n={n} seed={seed}")
        branches.add(bool(g.lda_fitted))
    assert branches  # (which branches occur is data; both are legitimate)


def test_rescore_rejects_sparse_keys_and_pct(gpu_required):
    from sage_amd._lib import SageHipError
    f, pk, npk, prk, npr = synthetic_features(1000, seed=12)
    with pytest.raises(SageHipError):
        rescore(f, Tolerance("ppm", -10.0, 10.0), pk, npk + 5, prk, npr)
    with pytest.raises(SageHipError):
        rescore(f, Tolerance("pct", -1.0, 1.0), pk, npk, prk, npr)
    g = rescore(f[:0], Tolerance("ppm", -10.0, 10.0), pk[:0], 0, prk[:0], 0)
    assert g.passing_spectrum == 0 and not g.lda_fitted


def test_search_then_rescore_end_to_end(gpu_required):
    """Features straight out of Scorer::score, keys from the host database, through the rescoring — the runner.rs flow."""
    fasta = synthetic_fasta(400, seed=31)
    params = DatabaseParameters(bucket_size=2048, enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                                static_mods={"C": 57.0215})
    host = params.build(fasta)
    dev = DeviceDatabase(host, 0)
    raw = synthetic_spectra(host, 3000, 32)
    sp = SpectrumProcessor(150, True, 0.0)
    batch = SpectrumBatch.from_spectra([sp.process(r) for r in raw])
    tol = Tolerance("ppm", -20.0, 20.0)
    scorer = Scorer(dev, ScorerParams(precursor_tol=tol, fragment_tol=Tolerance("ppm", -10.0, 10.0), report_psms=2))
    feats, counts = scorer.score(batch)
    flat = np.concatenate([feats[i, :counts[i]] for i in range(len(counts))])
    assert len(flat) > 1000 and (flat["label"] == -1).any()
    pk, npk, prk, npr = host.competition_keys(flat["peptide_idx"])
    g, o = compare(flat, tol, pk, npk, prk, npr, "end to end")  # (asserts lda_fitted equal: ims is constant here)
    assert g.passing_spectrum > 100


# ---- the predict_rt block (runner.rs:513-530) on the device --------------------------------------------------------------
def _close(got, exp, rtol, atol):
    """np.allclose over the finite and infinite values; where the oracle has a NaN the device must have one too, and nowhere else."""
    got, exp = np.asarray(got), np.asarray(exp)
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and np.allclose(got[~nan], exp[~nan], rtol=rtol, atol=atol)


RT_RTOL, RT_ATOL = 1e-3, 3e-4  # the bound of the four model outputs before the spreads were measured; now the cap of every bound


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def rt_tolerance(spread, exp_pred, exp_delta=None):
    """The bound of a model's predictions (or, with exp_delta, of |observed - prediction|) per element, from the oracle alone:
      * `spread`: the largest difference between the predictions of 16 oracle refits that differ in the order of the training
        rows and in the last 2 ulps of ln_1p (tests/rt_model_spread.py; profiles/rt_model_spread.json), times 16 — the device's
        blocked sums and its libm are one more draw from that family, and one more draw may pass the largest of 16, though not
        by such a factor;
      * 2 f32 ulps at the prediction: both sides round an f64 that differs by the above to f32;
      * for the delta, which is the f32 difference of the observation and that prediction, 2 ulps at the delta on top (its own
        rounding on either side); the prediction's error carries over in full, however small the delta is;
      * never more than RT_RTOL / RT_ATOL, the bound in force before: nothing weakens."""
    cap = RT_ATOL + RT_RTOL * np.abs(np.asarray(exp_pred if exp_delta is None else exp_delta, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        tol = 16.0 * spread + 2.0 * _ulp32(exp_pred) + (0.0 if exp_delta is None else 2.0 * _ulp32(exp_delta))
        return np.fmin(tol, cap)  # (fmin: an infinite or NaN spread leaves the cap)


def _within(got, exp, tol):
    """|got - exp| <= tol over the numbers (infinities equal); where the oracle has a NaN the device must have one too, and nowhere else."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    nan = np.isnan(exp)
    with np.errstate(invalid="ignore"):
        ok = (got == exp) | (np.abs(got - exp) <= tol)
    return np.array_equal(np.isnan(got), nan) and bool(np.all(ok[~nan]))


def rt_spread(name, case=None):
    """The measured spreads of a named world (profiles/rt_model_spread.json), or measured now from `case` for a world whose
    inputs exist only at run time."""
    import rt_model_spread
    return rt_model_spread.measure(*case) if case is not None else rt_model_spread.load()[name]


def compare_rt(f, n_files, off, seq, mono, context, spread=None):
    """spread: rt_spread() of the world — the four model outputs are then held to rt_tolerance(); without it (the order-free
    worlds of tests/test_gpu_rt_model_exact.py, which go on to demand equality) to RT_RTOL / RT_ATOL."""
    from sage_amd.api import predict_rt
    g = predict_rt(f, n_files, off, seq, mono)
    o = oracle_lib.predict_rt(f, n_files, off, seq, mono)
    assert np.array_equal(g.spectrum_q, o["spectrum_q"]), context  # integer counts, min: exact
    assert np.array_equal(g.alignments["max_rt"], o["alignments"][:, 0]), context
    assert _close(g.alignments["slope"], o["alignments"][:, 1], rtol=1e-5, atol=1e-6), context
    assert _close(g.alignments["intercept"], o["alignments"][:, 2], rtol=1e-5, atol=1e-6), context
    assert _close(g.aligned_rt, o["aligned_rt"], rtol=1e-5, atol=1e-6), context
    assert (g.rt_fitted, g.ims_fitted) == tuple(o["fitted"]), context
    # the normal equations are rank deficient (counts sum to the length, ...) and solved through a 1e-8 regulariser:
    # coefficients are noisy, predictions much less so — by how much is measured per world (rt_tolerance)
    sp = dict(rt=np.inf, ims=np.inf) if spread is None else spread
    for name, got, exp, tol in (
            ("predicted_rt", g.predicted_rt, o["predicted_rt"], rt_tolerance(sp["rt"], o["predicted_rt"])),
            ("delta_rt_model", g.delta_rt_model, o["delta_rt_model"], rt_tolerance(sp["rt"], o["predicted_rt"], o["delta_rt_model"])),
            ("predicted_ims", g.predicted_ims, o["predicted_ims"], rt_tolerance(sp["ims"], o["predicted_ims"])),
            ("delta_ims_model", g.delta_ims_model, o["delta_ims_model"], rt_tolerance(sp["ims"], o["predicted_ims"], o["delta_ims_model"]))):
        with np.errstate(invalid="ignore"):
            worst = np.nanmax(np.abs(got.astype(np.float64) - exp) / tol) if len(got) else 0.0
        print(f"{context} {name}: worst |device - oracle| / bound = {worst:.3g} (spread {sp['rt' if '_rt' in name else 'ims']:.3g})")
        assert _within(got, exp, tol), (context, name, np.nanmax(np.abs(got - exp)), worst)
    for fitted, got, exp in ((g.rt_fitted, g.rt_r2, o["r2"][0]), (g.ims_fitted, g.ims_r2, o["r2"][1])):
        if fitted:  # (all-zero ion mobilities: y_var == 0, r^2 = 1 - 0 / 0 on both sides)
            # (one training row: y_var == 0 and r^2 = 1 - sse / 0 = -inf on both sides; inf - inf is no number)
            assert (np.isnan(got) and np.isnan(exp)) or got == exp or abs(got - exp) < 1e-5, (context, got, exp)
    return g, o


@pytest.mark.parametrize("n,n_files,seed", [(20000, 3, 9), (500, 1, 10), (60000, 8, 11)])
def test_predict_rt_synthetic(gpu_required, n, n_files, seed):
    from sage_amd.synthetic import synthetic_rt_world
    f, off, seq, mono = synthetic_rt_world(n, n_files, seed=seed)
    import rt_model_spread
    g, _ = compare_rt(f, n_files, off, seq, mono, f"rt n={n} files={n_files}", rt_spread(rt_model_spread.synthetic_name(n, n_files, seed)))
    assert g.rt_fitted


def test_predict_rt_degenerate_inputs(gpu_required):
    from sage_amd._lib import SageHipError
    from sage_amd.api import predict_rt
    from sage_amd.synthetic import synthetic_rt_world
    f, off, seq, mono = synthetic_rt_world(4000, 2, seed=12, with_ims=False)  # no ion mobility: the IM model fits zeros
    compare_rt(f, 2, off, seq, mono, "no ims", rt_spread("degenerate/no_ims"))
    f0 = f.copy()
    f0["label"] = -1  # nothing to train on
    g, _ = compare_rt(f0, 2, off, seq, mono, "no targets", rt_spread("degenerate/no_targets"))
    assert not g.rt_fitted and np.all(g.delta_rt_model == np.float32(0.999))
    with pytest.raises(SageHipError):
        predict_rt(f, 1, off, seq, mono)  # file_id 1 with n_files 1


def _same_fields(a, b, context):
    """every output of two calls equal, NaNs matched; device_ms, the one field that is a measured time, aside"""
    for name, x in vars(a).items():
        y = getattr(b, name)
        if name == "alignments":  # a structured array: column by column
            assert all(_same(x[k], y[k]) for k in x.dtype.names), (context, name)
        elif name != "device_ms":
            assert _same(x, y), (context, name)


def test_without_the_pool_the_outputs_are_the_pooled_ones(gpu_required, monkeypatch):
    """SAGE_HIP_NO_POOL=1, read once per call: every scratch buffer of the call is a plain hipMalloc.  2 500 rows with a constant
    ims column cross the 1 024-element block of the blocked sums and the 1 024-row tile of the picked competitions' sequential sum."""
    from sage_amd.api import predict_rt
    from sage_amd.synthetic import synthetic_rt_world
    tol = Tolerance("ppm", -10.0, 10.0)
    calls = [(f"rescore n={n}", lambda a=synthetic_features(n, seed=seed, **kw): rescore(a[0], tol, *a[1:]))
             for n, seed, kw in ((300, 6, {}), (2500, 17, {"zero_ims": True}))]
    world = synthetic_rt_world(500, 1, seed=10)
    calls.append(("predict_rt", lambda: predict_rt(world[0], 1, *world[1:])))
    for context, call in calls:
        monkeypatch.delenv("SAGE_HIP_NO_POOL", raising=False)
        pooled = call()
        monkeypatch.setenv("SAGE_HIP_NO_POOL", "1")
        _same_fields(call(), pooled, context)


def test_search_predict_rescore_chain(gpu_required):
    """search -> predict_rt -> rescore with the model outputs as LDA features, against the oracle's chain"""
    from sage_amd.api import predict_rt
    fasta = synthetic_fasta(400, seed=41)
    params = DatabaseParameters(bucket_size=2048, enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                                static_mods={"C": 57.0215})
    host = params.build(fasta)
    dev = DeviceDatabase(host, 0)
    sp = SpectrumProcessor(150, True, 0.0)
    tol = Tolerance("ppm", -20.0, 20.0)
    scorer = Scorer(dev, ScorerParams(precursor_tol=tol, fragment_tol=Tolerance("ppm", -10.0, 10.0), report_psms=2))
    flat = []
    for file_id in range(2):
        raw = synthetic_spectra(host, 2000, 42 + file_id)
        batch = SpectrumBatch.from_spectra([sp.process(r) for r in raw])
        feats, counts = scorer.score(batch)
        part = np.concatenate([feats[i, :counts[i]] for i in range(len(counts))])
        part["file_id"] = file_id
        # synthetic spectra carry no retention time: give every peptide a reproducible one, stretched per file
        rng = np.random.default_rng(7)
        rt_of_pep = rng.uniform(5, 50, host.n_peptides).astype(np.float32)
        part["rt"] = rt_of_pep[part["peptide_idx"]] * np.float32(1.0 + 0.1 * file_id) + np.float32(2.0 * file_id)
        # ... and an ion mobility, so that no LDA column is constant: with constant columns the reference's elimination pivots
        # on rounding noise and neither side's coefficients mean anything
        ims_of_pep = rng.uniform(0.7, 1.2, host.n_peptides).astype(np.float32)
        part["ims"] = ims_of_pep[part["peptide_idx"]] + np.float32(0.1) * part["charge"] + rng.normal(0, 0.01, len(part)).astype(np.float32)
        flat.append(part)
    flat = np.concatenate(flat)
    off, seq, mono = host.feature_peptides(flat["peptide_idx"])
    # (the features come out of the device search: the spread of this world is measured here, from the oracle as everywhere)
    g, o = compare_rt(flat, 2, off, seq, mono, "chain", rt_spread("chain", (flat, 2, off, seq, mono)))
    pk, npk, prk, npr = host.competition_keys(flat["peptide_idx"])
    opt = dict(aligned_rt=o["aligned_rt"], delta_rt_model=o["delta_rt_model"], delta_ims_model=o["delta_ims_model"])
    compare(flat, tol, pk, npk, prk, npr, "chain rescore", **opt)
