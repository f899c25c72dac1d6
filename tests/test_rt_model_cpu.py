"""The order-free worlds of tests/rt_model_worlds.py, held to their premises with the oracle alone (no device):

  * the exactness budget — every design entry and training target is an integer on the world's grid and the sums of |x_j x_k|,
    |x_j y| stay below 2^53 units, which is what makes X^T X and X^T y exact in f64 in ANY order (measured: 2^39 - 2^47 units in
    the rt worlds, 2^20 - 2^33 in the im worlds).  Sum y^2 of the retention model is NOT exact (2^-58 units); it only enters r^2;
  * three readings agree: the numpy embeddings of tests/rt_model_reference.py with the oracle's on every peptide, the second
    reading with oracle_lib.predict_rt bit for bit, the oracle's beta with itself under permutations of the training rows;
  * sensitivity — a training row on a seam of the kernels' launch arithmetic that is dropped or counted twice changes the bits
    of f32 predictions, so equality with the device notices it.  The same mutants stay INSIDE the bound compare_rt() had
    (rtol 1e-3, atol 3e-4) in the large worlds: the worst of the 28 mutants moves a prediction by 0.051 of that bound in
    rt_exact/n65536 (16 384 training rows), 0.074 in rt_exact/n65537 and im_exact/n65536, 0.29 in im_exact/n65537 — that is
    the gap these worlds close (at 1 024 training rows the worst mutant reaches 1.4 - 3.9 bounds, most stay inside);
  * the preconditions of the arrangement: models fitted where intended, both clamps taken, the training set the one the
    arrangement assumed, the short lengths and odd residues present.

And profiles/rt_model_spread.json, the legitimate noise behind compare_rt()'s bounds on the worlds that are not order-free, is
recomputed for two worlds."""
import numpy as np
import pytest

import oracle_lib
import rt_model_reference as R
import rt_model_spread
import rt_model_worlds as W

GRID = {"rt": (0, 29), "im": (5, 10)}  # bits of the design's and the target's grid
SAMPLE = 4096  # rows whose predictions a mutant is compared on (any changed bit suffices)


def _oracle_model(w, o):
    """(design rows, target, clamp) of the world's order-free model as the oracle sees them"""
    f, _, off, seq, mono = w.case
    if w.kind == "rt":
        return oracle_lib.embed_rows(off, seq, mono), o["aligned_rt"].astype(np.float64), 1.0
    return oracle_lib.embed_rows(off, seq, mono, f["charge"]), f["ims"].astype(np.float64), 2.0


def _f32_predictions(rows, fit, hi):
    if fit is None:
        return None
    return R.bounded(R.dot_left_to_right(rows, fit[0]), np.zeros(len(rows), np.float32), hi)[0]


@pytest.mark.parametrize("name", W.WORLD_NAMES)
def test_exactness_budget(name):
    w, o, r = R.readings(name)
    rows, y, _ = _oracle_model(w, o)
    train = w.train
    xb, yb = GRID[w.kind]
    xi, yi = R.to_grid(rows[train], xb), R.to_grid(y[train], yb)  # raises unless the scaling is exact
    assert np.array_equal(xi * 2.0 ** -xb, rows[train]) and np.array_equal(yi * 2.0 ** -yb, y[train])
    ax, ay = np.abs(xi).astype(np.float64), np.abs(yi).astype(np.float64)  # (sums of magnitudes: an upper bound needs no exactness)
    budget = max((ax.T @ ax).max(), (ax.T @ ay).max())
    print(f"{name}: n={w.n} nb={w.nb} per={w.per} train={int(train.sum())} budget 2^{np.log2(max(budget, 1)):.1f} units, "
          f"seams {dict((k, w.seams[k]) for k in w.occupied)}")
    assert budget < 2.0 ** 52, name  # (one bit of margin for the float sum of magnitudes itself)
    assert r["budget"] == int(budget), name  # the second reading's integer count of the same thing
    if w.kind == "rt":
        assert np.all(w.case[4] == 0.0) and np.all(rows[:, R.RT_D - 2] == 0.0), name  # ln_1p(0) == 0 on every libm
        assert np.abs(o["aligned_rt"][train]).min() >= 2.0 ** -6, name  # f32 lsb >= 2^-29


@pytest.mark.parametrize("name", W.WORLD_NAMES)
def test_embeddings_agree(name):
    w, _, _ = R.readings(name)
    f, _, off, seq, mono = w.case
    for mine, theirs in ((R.rt_embed(off, seq, mono), oracle_lib.embed_rows(off, seq, mono)),
                         (R.im_embed(off, seq, mono, f["charge"]), oracle_lib.embed_rows(off, seq, mono, f["charge"]))):
        assert mine.shape == theirs.shape and np.array_equal(mine, theirs), (name, np.argwhere(mine != theirs)[:5])
    # ... and the oracle's rows are its embedding of one sequence at a time (every short peptide, and a sample of the rest)
    lens = np.diff(off.astype(np.int64))
    pick = np.unique(np.concatenate([np.flatnonzero(lens <= 4)[:64], np.linspace(0, w.n - 1, 64).astype(np.int64)]))
    rt_rows, im_rows = R.rt_embed(off, seq, mono), R.im_embed(off, seq, mono, f["charge"])
    for i in pick:
        s = seq[int(off[i]):int(off[i + 1])].tobytes().decode()
        assert np.array_equal(oracle_lib.rt_embed(s, float(mono[i])), rt_rows[i]), (name, i, s)
        assert np.array_equal(oracle_lib.im_embed(s, float(mono[i]), int(f["charge"][i])), im_rows[i]), (name, i, s)


@pytest.mark.parametrize("name", W.WORLD_NAMES)
def test_second_reading_equals_oracle(name):
    w, o, r = R.readings(name)
    pred, delta, k = R.model_fields(w.kind)
    assert np.array_equal(r["spectrum_q"], o["spectrum_q"]), name
    assert np.array_equal(r["alignments"], o["alignments"]), name
    assert np.array_equal(r["aligned_rt"], o["aligned_rt"]), name
    assert r["fitted"] == bool(o["fitted"][k]), name
    assert np.array_equal(r["predicted"], o[pred]), (name, int(np.sum(r["predicted"] != o[pred])))
    assert np.array_equal(r["delta"], o[delta]), name
    if r["fitted"] and np.isfinite(o["r2"][k]):
        # im worlds: y_var is exact too, only the SSE sum has an order (the same on both sides here); rt worlds: sum y^2 rounds
        # once here and once per row in the oracle
        assert abs(r["r2"] - o["r2"][k]) <= (1e-12 * abs(o["r2"][k]) if w.kind == "im" else 1e-5), (name, r["r2"], o["r2"][k])


@pytest.mark.parametrize("name", W.WORLD_NAMES)
def test_oracle_beta_is_order_free(name):
    w, o, _ = R.readings(name)
    rows, y, _ = _oracle_model(w, o)
    t = np.flatnonzero(w.train)
    base = oracle_lib.linreg_fit(rows[t], y[t])
    rng = np.random.default_rng(17)
    for _ in range(4):
        p = rng.permutation(t)
        again = oracle_lib.linreg_fit(rows[p], y[p])
        assert (base is None) == (again is None), name
        if base is not None:
            assert np.array_equal(base[0], again[0]), name  # bit for bit


@pytest.mark.parametrize("name", W.WORLD_NAMES)
def test_a_lost_or_doubled_seam_row_changes_predictions(name):
    w, o, _ = R.readings(name)
    rows, y, hi = _oracle_model(w, o)
    t = np.flatnonzero(w.train)
    base = oracle_lib.linreg_fit(rows[t], y[t])
    if name == "rt_exact/one_train":
        assert base is None  # one row: the elimination fails on both sides; this world holds the flags and the count, not the fit
        return
    assert base is not None, name
    assert len(w.occupied) >= 1, name
    sample = rows[:SAMPLE]
    p0 = _f32_predictions(sample, base, hi)
    worst = 0.0
    for seam in w.occupied:
        i = w.seams[seam]
        for what, sel in (("lost", t[t != i]), ("doubled", np.concatenate([t, [i]]))):
            fit = oracle_lib.linreg_fit(rows[sel], y[sel]) if len(sel) else None
            p = _f32_predictions(sample, fit, hi)
            assert p is None or not np.array_equal(p.view(np.uint32), p0.view(np.uint32)), (name, seam, i, what)
            if p is not None:
                with np.errstate(invalid="ignore"):
                    worst = max(worst, float(np.nanmax(np.abs(p.astype(np.float64) - p0) / (3e-4 + 1e-3 * np.abs(p0)))))
    print(f"{name}: {2 * len(w.occupied)} mutants, worst |change| / (3e-4 + 1e-3 |p|) = {worst:.3g}")


@pytest.mark.parametrize("name", W.WORLD_NAMES)
def test_world_preconditions(name):
    w, o, _ = R.readings(name)
    f, n_files, off, seq, mono = w.case
    pred, _, k = R.model_fields(w.kind)
    train = (f["label"] == 1) & (o["spectrum_q"] <= np.float32(0.01))
    assert np.array_equal(train, w.train), name  # the training set is the one the arrangement assumed
    assert (w.nb, w.per) == W.launch(w.n) and w.n == len(f) and n_files == W.N_FILES
    tail = name.endswith("tail300")
    one = name.endswith("one_train")
    assert int(train.sum()) == (1 if one else max(100, w.n // 4)), name
    if one:
        assert w.occupied == ("block_start",) and train[w.per], name
    elif tail:
        assert not train[-300:].any() and set(w.occupied) == {s for s, i in w.seams.items() if i < w.n - 300}, name
        assert len(w.occupied) >= 8, name
    else:
        assert set(w.occupied) == set(w.seams), name  # every seam holds a training row
        for i in (0, 15, 16, w.per - 1, w.n - 1, 63, 64) + ((w.per,) if w.per < w.n else ()):
            assert train[i], (name, i)
    assert bool(o["fitted"][k]) == (name != "rt_exact/one_train"), name
    lens = np.diff(off.astype(np.int64))
    assert np.array_equal(lens, f["peptide_len"]), name
    if w.kind == "rt":
        assert lens.min() == 1 and lens.max() == 40, name
    else:
        assert set(np.unique(lens)) <= {1, 2, 4, 8, 16, 32} and set(np.unique(f["charge"])) == {1, 2, 4}, name
        assert np.all(mono % 1000 == 0) and np.all(f["ims"] * 1024 == np.rint(f["ims"] * 1024)), name
        assert (np.ptp(mono) == 0) == name.endswith("mono0"), name
        inside = (f["ims"] >= 0.5) & (f["ims"] <= 1.5)
        assert inside.mean() > 0.9 and (not w.clamps or not inside.all()), name  # the bulk; a few leave it with the law
    if not one:
        short = (1, 2, 3, 4) if w.kind == "rt" else (1, 2, 4)
        assert set(short) <= set(lens[train]), name  # the cterm branches of both embeddings, among the training rows
        assert {ord(c) for c in "XBUO"} <= set(seq), name
    if w.clamps:
        hi = 1.0 if w.kind == "rt" else 2.0
        assert (o[pred] == 0.0).any() and (o[pred] == np.float32(hi)).any(), name
        assert ((o[pred] > 0.0) & (o[pred] < np.float32(hi))).mean() > 0.99, name
        if w.kind == "im":  # ... and the retention model's clamps in the same worlds
            assert (o["predicted_rt"] == 0.0).any() and (o["predicted_rt"] == 1.0).any() and o["fitted"][0], name


def test_seams_follow_the_launch_arithmetic():
    for n, nb, per in ((255, 1, 255), (256, 1, 256), (257, 2, 129), (4097, 17, 241), (65536, 256, 256), (65537, 256, 257)):
        assert W.launch(n) == (nb, per)
        s = W.seams(n)
        assert s["n-1"] == s["last_block_hi-1"] == n - 1 and s["last_block_start"] == ((n - 1) // per) * per
        assert ("block_start" in s) == (nb > 1)
    assert W.seams(4097)["last_stage_start"] == 16 * 241 + 240 and 241 % 16 != 0 and 256 % 16 == 0


def test_regulariser_ladder_depends_on_the_order_of_the_sums():
    """Why no bound on predictions can hold everywhere: gauss.rs:42-51 retries the elimination with eps = 1e-8, 1e-7, ... 1.0
    until left_solved() (an exact 1.0 on the diagonal, no off-diagonal above 1e-8) accepts it, and which eps that is can hang on
    the last bits of X^T X.  On this world's mobility model the reference's sequential sums are accepted at 1e-8 and the same
    products summed per 241-row block, then over the blocks — the device's order, and as legitimate as any rayon split — only
    at 1.0: predictions 0.053 apart, both from the oracle's own solve.  (The worlds under test avoid the regime: ims == 0 in
    rt worlds.)"""
    w = W.world(W.LADDER_WORLD)
    f, _, off, seq, mono = w.case
    rows, y = oracle_lib.embed_rows(off, seq, mono, f["charge"]), f["ims"].astype(np.float64)
    d = rows.shape[1]
    seq_a, seq_b, blk_a, blk_b = np.zeros((d, d)), np.zeros(d), np.zeros((d, d)), np.zeros(d)
    for lo in range(0, w.n, w.per):
        a, b = np.zeros((d, d)), np.zeros(d)
        for i in np.flatnonzero(w.train[lo:lo + w.per]) + lo:
            outer, xy = np.outer(rows[i], rows[i]), rows[i] * y[i]
            a, b, seq_a, seq_b = a + outer, b + xy, seq_a + outer, seq_b + xy
        blk_a, blk_b = blk_a + a, blk_b + b
    assert np.abs(blk_a - seq_a).max() <= 1e-15 * np.abs(seq_a).max() * w.per  # the same matrix but for the last bits
    p_seq, p_blk = (np.clip(rows @ oracle_lib.gauss_solve(a, b), 0.0, 2.0) for a, b in ((seq_a, seq_b), (blk_a, blk_b)))
    ridge = lambda eps: np.clip(rows @ np.linalg.solve(seq_a + eps * np.eye(d), seq_b), 0.0, 2.0)  # noqa: E731
    assert np.abs(p_seq - ridge(1e-8)).max() < 1e-6 and np.abs(p_blk - ridge(1.0)).max() < 1e-6
    assert np.abs(p_seq - p_blk).max() > 0.05


def test_spread_file_is_current():
    table = rt_model_spread.load()
    cases = rt_model_spread.cases()
    assert set(table) == set(cases)
    for name in (rt_model_spread.synthetic_name(500, 1, 10), "rt/n257"):
        with np.errstate(invalid="ignore", divide="ignore"):
            now = rt_model_spread.measure(*cases[name], seed=2)  # (other draws than the file's)
        for key in ("rt", "ims"):
            assert table[name][key] > 0 and table[name][key] / 4 <= now[key] <= table[name][key] * 4, (name, key, now, table[name])
        assert (now["n"], now["train"]) == (table[name]["n"], table[name]["train"])
