"""Edge-case inputs of the post-search stages (sage_hip_rescore, sage_hip_predict_rt): ties, block / tile seams, non-finite
values, degenerate competitions.  Plain numpy on top of synthetic_features / synthetic_rt_world, fixed seeds.

    RESCORE_CASES[name] = (features, peptide_key, n_peptide_keys, protein_key, n_protein_keys, options, ref_leg)
    RT_CASES[name]      = (features, n_files, seq_off, seq, monoisotopic)

`options` holds the precursor tolerance under "tol" and, where given, the three model-input arrays.  `ref_leg` says whether
the case is also held to the oracle's reference-order mode (det=False): tests/test_rescore_edges_cpu.py proves for every case
that the flag is a fact about the data (the oracle's two modes meet compare()'s thresholds against each other, or they do
not), never a convenience.

The sizes come from the partition sizes of rescore.hip as the design states them, written down here on purpose instead of
being imported from the product: 256 rows per row-parallel block, 128 rows per LDA tile (two 64-row masks, double
buffered), 1024 elements per block of the blocked sums (per class), 1024 rows per tile of the sequential f32 sum of a picked
competition (over the rows PRESENT in it), 512 x 256 = 131 072 rows per trip of the grid-stride reductions.

Also here, because the CPU and the GPU tests share them: numpy readings of the q-value pass and of the picked competition,
written from the reference's ml/qvalue.rs and fdr.rs, not from the oracle.
"""
import numpy as np

from sage_amd.api import Tolerance
from sage_amd.synthetic import synthetic_features, synthetic_rt_world

NO_KEY = 0xFFFFFFFF
LDA_TILE, CLASS_BLOCK, ROW_TILE, GRID_TRIP = 128, 1024, 1024, 512 * 256
PPM = Tolerance("ppm", -10.0, 10.0)
DA = Tolerance("da", -500.0, 100.0)


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _dense(keys):
    """Renumber the keys in use 0..k-1 (NO_KEY stays); returns (keys, k)."""
    keys = np.asarray(keys, dtype=np.uint32)
    out = np.full(len(keys), NO_KEY, dtype=np.uint32)
    live = keys != NO_KEY
    used, inv = np.unique(keys[live], return_inverse=True)
    out[live] = inv.astype(np.uint32)
    return out, len(used)


def _take(table, rows):
    """The sub-table of the given rows (in that order), competition keys renumbered."""
    f, pk, _, prk, _ = table
    pk, n_pk = _dense(pk[rows])
    prk, n_pr = _dense(prk[rows])
    return f[rows].copy(), pk, n_pk, prk, n_pr


def _model_inputs(n, seed):
    rng = np.random.default_rng(seed)
    return dict(aligned_rt=rng.uniform(0, 1, n).astype(np.float32),
                delta_rt_model=np.abs(rng.normal(0, 0.05, n)).astype(np.float32),
                delta_ims_model=np.abs(rng.normal(0, 0.02, n)).astype(np.float32))


def _case(table, ref_leg, tol=PPM, **opt):
    f, pk, n_pk, prk, n_pr = table
    for k, n_k in ((pk, n_pk), (prk, n_pr)):  # the device indexes its per-key arrays with these: keep them in range
        live = k[k != NO_KEY]
        assert k.dtype == np.uint32 and len(k) == len(f) and (len(live) == 0 or int(live.max()) < n_k)
        assert len(np.unique(live)) == n_k
    return f, pk, n_pk, prk, n_pr, dict(opt, tol=tol), ref_leg


def competition_rows(key, decoy):
    """Rows present in a picked competition: one per (key, side) that at least one feature belongs to."""
    key, decoy = np.asarray(key), np.asarray(decoy, dtype=bool)
    live = key != NO_KEY
    return len(np.unique(key[live].astype(np.int64) * 2 + decoy[live]))


# ---- ties --------------------------------------------------------------------------------------------------------------------
def repeated_rows(seed, opt_seed=None, **kw):
    """3000 base rows, each three times in shuffled positions: every discriminant is shared by three rows."""
    base = synthetic_features(3000, seed=seed, **kw)
    rows = np.random.default_rng(seed + 1000).permutation(np.repeat(np.arange(3000), 3))
    table = _take(base, rows)
    opt = {} if opt_seed is None else {k: v[rows] for k, v in _model_inputs(3000, opt_seed).items()}
    return table, opt


def twins(seed, opt_seed):
    """3000 base rows, each twice, with the same model inputs; under the peptide keys without a true hit the second copy has
    its label flipped (same peptide and protein key).  The two sides of those keys hold the same scores, so the best target
    EQUALS the best decoy and `reverse >= forward` (fdr.rs:47-49) decides — the decoy wins.  Under the keys with a true hit the
    copy keeps its label, so that something still passes 1 %."""
    f, pk, n_pk, prk, n_pr = synthetic_features(3000, seed=seed)
    has_true = np.zeros(n_pk, bool)
    has_true[pk[(f["label"] == 1) & (f["hyperscore"] > 24)]] = True
    g = f.copy()
    g["label"] = np.where(has_true[pk], f["label"], -f["label"])
    rows = np.random.default_rng(seed + 1000).permutation(2 * len(f))
    table = _take((np.concatenate([f, g]), np.concatenate([pk, pk]), n_pk, np.concatenate([prk, prk]), n_pr), rows)
    return table, {k: np.concatenate([v, v])[rows] for k, v in _model_inputs(3000, opt_seed).items()}


def quantised_poisson(seed, n=4000):
    """`poisson` rounded to whole numbers on a table without ion mobility whose fit fails (test_rescore_edges_cpu.py checks
    that it does): the heuristic discriminant ln_1p(-poisson) + longest_y_pct / 3 is then built from discrete fields only."""
    f, *keys = synthetic_features(n, seed=seed, zero_ims=True)
    f["poisson"] = np.round(f["poisson"])
    return (f, *keys)


# ---- seams -------------------------------------------------------------------------------------------------------------------
def class_counts(seed, n_decoy, n_target, **kw):
    """A table with exactly n_decoy decoys and n_target targets: the first so many rows of each class of a larger draw, in
    their original order (labels chosen by position; the scores keep the structure of the draw, so the model still fits)."""
    base = synthetic_features(2 * (n_decoy + n_target) + 2000, seed=seed, **kw)
    decoy = base[0]["label"] == -1
    rows = np.sort(np.concatenate([np.flatnonzero(decoy)[:n_decoy], np.flatnonzero(~decoy)[:n_target]]))
    assert len(rows) == n_decoy + n_target
    return _take(base, rows)


def _keys_with_rows(decoy, m, takes_part, rng):
    """Competition keys under which exactly m rows (key, side) are present: m // 3 keys with both sides (2 rows each), the
    rest one-sided keys (1 row each), key ids shuffled.  Features outside `takes_part` get NO_KEY."""
    both = m // 3
    single = m - 2 * both
    d_only = single // 5
    n_keys = both + single
    ids = rng.permutation(n_keys).astype(np.uint32)
    slots = {True: np.concatenate([ids[:both], ids[both:both + d_only]]), False: np.concatenate([ids[:both], ids[both + d_only:]])}
    key = np.full(len(decoy), NO_KEY, dtype=np.uint32)
    for side in (True, False):
        rows = np.flatnonzero((decoy == side) & takes_part)
        assert len(rows) >= len(slots[side]) > 0, (m, side, len(rows))
        key[rows] = slots[side][rng.permutation(len(rows)) % len(slots[side])]  # (every slot is hit: more rows than slots)
    return key, n_keys


def competition_seam(seed, m_peptide, m_protein):
    """3000 rows whose peptide competition has exactly m_peptide rows present and whose protein competition m_protein."""
    f, *_ = synthetic_features(3000, seed=seed)
    decoy = f["label"] == -1
    rng = np.random.default_rng(seed + 1000)
    pk, n_pk = _keys_with_rows(decoy, m_peptide, np.ones(len(f), bool), rng)
    if m_protein <= 2:  # one protein, seen from the target side only (1 row) or from both sides (2 rows)
        part = (rng.random(len(f)) < 0.5) & (~decoy if m_protein == 1 else True)
        prk, n_pr = np.where(part, 0, NO_KEY).astype(np.uint32), 1
    else:
        prk, n_pr = _keys_with_rows(decoy, m_protein, rng.random(len(f)) < 0.95, rng)
    return f, pk, n_pk, prk, n_pr


def past_one_grid_trip(seed):
    """131 072 + 300 rows, the largest and the smallest delta_mass of the whole table among the last 300: a min / max
    reduction that stops after one trip of its grid-stride loop gets another mass-error KDE grid."""
    f, *keys = synthetic_features(GRID_TRIP + 300, seed=seed)
    f["delta_mass"][-7] = 12.5
    f["delta_mass"][-200] = -13.25
    assert f["delta_mass"][:GRID_TRIP].max() < 12.5 and f["delta_mass"][:GRID_TRIP].min() > -13.25
    return (f, *keys)


# ---- non-finite values, degenerate competitions ---------------------------------------------------------------------------------
def with_values(table, field, values):
    f, *keys = table
    f = f.copy()
    f[field][:len(values)] = values
    return (f, *keys)


def one_sided_keys(seed):
    f, pk, _, prk, _ = synthetic_features(3000, seed=seed)
    decoy = (f["label"] == -1).astype(np.uint32)
    pk, n_pk = _dense(pk * 2 + decoy)
    prk, n_pr = _dense(np.where(prk == NO_KEY, NO_KEY, prk * 2 + decoy))
    return f, pk, n_pk, prk, n_pr


def single_label(seed, label):
    """Every row of the other class, but row 1234."""
    f, *keys = synthetic_features(3000, seed=seed)
    f["label"] = -label
    f["label"][1234] = label
    return (f, *keys)


# (n, seed, ref_leg)
LDA_SEAM_SIZES = [(1, 101, True), (2, 102, True), (3, 103, True), (63, 163, True), (64, 164, True), (65, 215, True),
                  (127, 227, True), (128, 228, True), (129, 229, True), (255, 455, True), (256, 406, True), (257, 457, True),
                  (383, 483, True), (385, 485, True)]

TIE_CASES = ("tie/repeat3", "tie/repeat3_const", "tie/repeat3_zero_ims", "tie/repeat3_no_decoys", "tie/twins", "tie/quantised_poisson", "da/repeat3")
HEURISTIC_CASES = ("tie/repeat3_no_decoys", "tie/quantised_poisson", "nonfinite/poisson")
# name -> (decoys, targets, seed): one class at the seam, the other no multiple of the block
CLASS_SEAMS = {f"class_seam/d{d}_t{t}": (d, t, seed) for d, t, seed in ((1023, 1977, 51), (1024, 1977, 52), (1025, 1977, 53),
                                                                        (1500, 1023, 54), (1500, 1024, 55), (1500, 1025, 56))}
# name -> (rows present in the peptide competition, in the protein competition, seed)
COMPETITION_SEAMS = {f"comp_seam/pep{a}_prot{b}": (a, b, seed) for a, b, seed in ((1023, 1, 61), (1024, 2, 62), (1025, 2048, 63),
                                                                                 (2048, 1025, 64), (2049, 1023, 65))}


def _build_rescore_cases():
    c = {}
    # Without the three model-input arrays the last two columns of the design are constant (the defaults 0.999): the elimination
    # then pivots on rounding noise, the coefficients of the two modes of the oracle have nothing to do with each other and
    # compare() holds the device to the reference-order mode in the fit-or-heuristic decision only.  So the families that are to
    # carry that leg come WITH model inputs; the *_const cases and the non-finite / degenerate ones keep the defaults.
    # -- ties.  (The reference sorts unstably and walks a hash map; the order inside a tie is the contract stated in the header of
    #    oracle/rescore_oracle.cpp: stable sorts, rows in key-ascending / forward-before-reverse order.)
    table, opt = repeated_rows(41, opt_seed=141)
    c["tie/repeat3"] = _case(table, True, **opt)
    c["tie/repeat3_const"] = _case(repeated_rows(41)[0], True)
    c["tie/repeat3_zero_ims"] = _case(repeated_rows(42, zero_ims=True)[0], True)
    c["tie/repeat3_no_decoys"] = _case(repeated_rows(43, decoy_frac=0.0)[0], True)
    table, opt = twins(44, opt_seed=144)
    c["tie/twins"] = _case(table, True, **opt)
    c["tie/quantised_poisson"] = _case(quantised_poisson(3), True)
    table, opt = repeated_rows(45, opt_seed=46, ppm=False)
    c["da/repeat3"] = _case(table, True, tol=DA, **opt)
    # -- seams of the LDA tile, its double buffer and the wave masks (and of the 256-row blocks)
    for n, seed, ref_leg in LDA_SEAM_SIZES:
        c[f"lda_seam/n{n}"] = _case(synthetic_features(n, seed=seed), ref_leg, **_model_inputs(n, seed + 1000))
        c[f"lda_seam_const/n{n}"] = _case(synthetic_features(n, seed=seed), True)
    # -- per-class counts at the block of the blocked sums; the other class is no multiple of it
    for name, (n_d, n_t, seed) in CLASS_SEAMS.items():
        c[name] = _case(class_counts(seed, n_d, n_t), True, **_model_inputs(n_d + n_t, seed + 1000))
    c["da/class_seam_d1025_t1977"] = _case(class_counts(57, 1025, 1977, ppm=False), True, tol=DA, **_model_inputs(1025 + 1977, 58))
    # -- rows present in the competitions at the tile of the sequential sum
    for name, (m_pep, m_prot, seed) in COMPETITION_SEAMS.items():
        c[name] = _case(competition_seam(seed, m_pep, m_prot), True, **_model_inputs(3000, seed + 1000))
    c["grid_seam/n131372"] = _case(past_one_grid_trip(131372), False)  # det=True leg only: one oracle pass costs seconds here
    # -- non-finite and degenerate values
    base = synthetic_features(2000, seed=71)
    c["nonfinite/hyperscore_nan"] = _case(with_values(base, "hyperscore", [np.nan]), True)
    c["nonfinite/hyperscore_inf"] = _case(with_values(base, "hyperscore", [np.inf]), True)
    c["nonfinite/hyperscore_zero"] = _case(with_values(base, "hyperscore", [0.0]), True)
    c["nonfinite/delta_mass_nan"] = _case(with_values(base, "delta_mass", [np.nan]), True)
    c["nonfinite/ims_inf"] = _case(with_values(base, "ims", [np.inf]), True)
    c["nonfinite/rt_inf"] = _case(with_values(base, "rt", [np.inf]), True)
    c["nonfinite/ms2_intensity_inf"] = _case(with_values(base, "ms2_intensity", [np.inf]), True)
    # ln_1p(-poisson) of these on the heuristic path: 0, 0, ln 0.5, -inf, NaN, NaN, NaN
    c["nonfinite/poisson"] = _case(with_values(synthetic_features(4000, seed=3, zero_ims=True), "poisson",
                                               [0.0, -0.0, 0.5, 1.0, 2.0, np.inf, np.nan]), True)
    # -- degenerate competitions
    f, pk, n_pk, prk, n_pr = synthetic_features(3000, seed=81)
    c["degenerate/all_proteins_shared"] = _case((f, pk, n_pk, np.full(len(f), NO_KEY, np.uint32), 0), True)
    c["degenerate/one_key"] = _case((f, np.zeros(len(f), np.uint32), 1, np.zeros(len(f), np.uint32), 1), True)
    c["degenerate/one_sided_keys"] = _case(one_sided_keys(82), True)
    c["degenerate/one_decoy"] = _case(single_label(83, -1), True)
    c["degenerate/one_target"] = _case(single_label(84, 1), True)
    f, *keys = synthetic_features(3000, seed=85)
    f["label"] = -1
    c["degenerate/all_decoys"] = _case((f, *keys), True)
    return c


# ---- the predict_rt block ----------------------------------------------------------------------------------------------------
RT_257_SEED = 457


def _build_rt_cases():
    c = {}
    for n, seed in ((1, 201), (2, 202), (70, 270)):  # no PSM passes 1 %: neither model is fitted
        c[f"rt/n{n}"] = _rt(n, 1, seed)
    f, _, off, seq, mono = _rt(257, 1, RT_257_SEED)
    decoys = np.flatnonzero(f["label"] == -1)
    f["label"][decoys[decoys % 16 != 0]] = 1  # few decoys: 1 % needs 100 targets ahead of the second decoy, of 257 rows
    c["rt/n257"] = (f, 1, off, seq, mono)
    c["rt/files70"] = _rt(6000, 70, 203)  # more files than the 64 blocks the per-file sums are capped at
    f, off, seq, mono = synthetic_rt_world(3000, 2, seed=204)
    c["rt/unused_file_id"] = (f, 3, off, seq, mono)
    f, _, off, seq, mono = _rt(4000, 3, 205)
    f["rt"][f["file_id"] == 1] = 0.0  # max_rt == 0: 0 / 0 in the matrix and in aligned_rt
    c["rt/zero_rt_file"] = (f, 3, off, seq, mono)
    f, _, off, seq, mono = _rt(4000, 2, 206)
    f["file_id"][:5] = 0  # (file 1 keeps an ordinary maximum)
    f["rt"][:5] = [np.nan, np.inf, -1.0, 0.0, 5e9]  # `rt.ceil() as u32` saturates at 2^32 - 1, NaN and negatives give 0
    c["rt/rt_specials"] = (f, 2, off, seq, mono)
    f, _, off, seq, mono = _rt(4000, 2, 207)
    f["poisson"] = np.round(f["poisson"])
    c["rt/quantised_poisson"] = (f, 2, off, seq, mono)
    f, _, off, seq, mono = _rt(4000, 2, 208)
    seq = seq.copy()
    rng = np.random.default_rng(209)
    at = rng.choice(len(seq), size=len(seq) // 20, replace=False)
    seq[at] = np.frombuffer(b"XBU", dtype=np.uint8)[rng.integers(0, 3, len(at))]  # X, B: outside VALID_AA (index 0); U: inside
    c["rt/odd_residues"] = (f, 2, off, seq, mono)
    f, _, off, seq, mono = _rt(4000, 2, 210)
    f["file_id"] = (f["peptide_idx"] // 2) % 2  # every peptide in one file only: one finite entry per matrix row
    c["rt/one_file_per_peptide"] = (f, 2, off, seq, mono)
    return c


def _rt(n, n_files, seed):
    with np.errstate(invalid="ignore"):  # (one peptide: its retention normalises to 0 / 0, a NaN rt — kept, it is an input too)
        f, off, seq, mono = synthetic_rt_world(n, n_files, seed=seed)
    return f, n_files, off, seq, mono


RESCORE_CASES = _build_rescore_cases()
RT_CASES = _build_rt_cases()


# ---- numpy readings of the reference ---------------------------------------------------------------------------------------------
def total_order_f32(x):
    """Integers whose ascending order is f32::total_cmp."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def descending_stable_order(scores):
    """Best first in the f32 total order, ascending row index inside a tie."""
    return np.argsort(-total_order_f32(scores), kind="stable").astype(np.uint32)


def spectrum_q_of(order, decoy):
    """ml/qvalue.rs:8-36 over the rows in `order`; q-values in input order."""
    d = np.asarray(decoy, dtype=bool)[order]
    with np.errstate(divide="ignore"):
        q = (1 + np.cumsum(d)).astype(np.float32) / np.cumsum(~d).astype(np.float32)
    q = np.minimum(np.minimum.accumulate(q[::-1])[::-1], np.float32(1.0))
    out = np.empty(len(order), np.float32)
    out[order] = q
    return out


def picked_q_of(key, n_keys, decoy, score, posterior_error_of):
    """fdr.rs:42-120 and the write-back of :146-148 / :179-185 over dense keys.  `posterior_error_of(winner_scores,
    winner_is_decoy, queries)` is the fitted KDE of :51-57 evaluated at the queries (f64).  q-values in input order."""
    key, decoy = np.asarray(key), np.asarray(decoy, dtype=bool)
    score = np.asarray(score, dtype=np.float32)
    out = np.ones(len(key), np.float32)
    live = key != NO_KEY
    if n_keys == 0 or not live.any():
        return out
    fmin = np.finfo(np.float32).min
    best = np.full((n_keys, 2), fmin, np.float32)  # [key][0 forward | 1 reverse]; f32::max ignores a NaN operand
    present = np.zeros((n_keys, 2), bool)
    side = decoy.astype(np.int64)
    np.fmax.at(best, (key[live].astype(np.int64), side[live]), score[live])
    present[key[live].astype(np.int64), side[live]] = True
    seen = present.any(axis=1)
    winner = np.fmax(best[:, 0], best[:, 1])[seen].astype(np.float64)
    winner_decoy = (best[:, 1] >= best[:, 0])[seen]  # a tie goes to the decoy
    row_key, row_side = np.nonzero(present)  # key ascending, forward before reverse
    row_score = best[row_key, row_side]
    srt = np.argsort(-total_order_f32(row_score), kind="stable")
    row_key, row_side, row_score = row_key[srt], row_side[srt], row_score[srt]
    pep = np.asarray(posterior_error_of(winner, winner_decoy, row_score.astype(np.float64))).astype(np.float32)
    q = np.empty(len(pep), np.float32)
    dsum, target = np.float32(1.0), np.float32(0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(len(pep)):
            dsum = np.float32(dsum + pep[j])
            if row_side[j] == 0:
                target = np.float32(target + np.float32(1.0))
            q[j] = dsum / target
    qmin = np.float32(1.0)
    side_q = np.ones((n_keys, 2), np.float32)
    for j in range(len(q) - 1, -1, -1):
        qmin = qmin if np.isnan(q[j]) else min(qmin, q[j])  # f32::min: a NaN q leaves q_min as it is
        side_q[row_key[j], row_side[j]] = qmin
    out[live] = side_q[key[live].astype(np.int64), side[live]]
    return out
