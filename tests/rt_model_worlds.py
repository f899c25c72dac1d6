"""Order-free worlds for the retention-time and ion-mobility models of the predict_rt block (xtx_kernel, fold_partials_kernel,
predict_kernel of sage_amd/csrc/rt_model.hip and the host gauss_solve of rescore.hip).

The normal equations of both models are rank deficient and solved through a 1e-8 regulariser, so a last-bit difference in
X^T X grows, and a comparison of predictions needs a tolerance that also lets a lost training row through.  Here every entry of
one model's design matrix and of its target sits on a coarse dyadic grid:

  rt_exact/*   monoisotopic mass 0 (ln_1p(0) == 0): the retention design is residue counts, the length and 1 — small integers;
               the target, aligned_rt, is an f32 of magnitude >= 2^-6, i.e. a multiple of 2^-29;
  im_exact/*   peptide lengths in {1, 2, 4, 8, 16, 32}, charges in {1, 2, 4}, masses in {0, 1000, 2000, 3000, 4000}: the
               mobility design (counts, counts / length, z, 1 / z, mass / 1000, mass / z / 1000) is multiples of 2^-5; the target,
               ims, is multiples of 2^-10.

Every product x_j * x_k and x_j * y is then a multiple of one unit, and while the sum of their magnitudes stays below 2^53 units
(tests/test_rt_model_cpu.py asserts the budget) every partial sum of X^T X and X^T y is exact in f64 IN ANY ORDER: the device's
blocked sums and the reference's sequential ones are the same numbers, the two Gauss-Jordan solves get the same input, and every
prediction must be bit-equal.  Equality does notice a row that is lost, counted twice or embedded wrongly.

The PSM tables come from sage_amd.synthetic.synthetic_rt_world (labels, peptide keys, files, scores); sequences, retention
times, mobilities, masses and the poisson ranking are rewritten here.  The ranking is built so that the training set (label == 1
&& spectrum_q <= 0.01) is known by construction, and the rows are then reordered to put training rows on the seams of the
kernels' launch arithmetic (seams() below restates that arithmetic; nothing is hard-coded per size).
"""
import functools
from collections import namedtuple

import numpy as np

from sage_amd.synthetic import _AA, _FREQ, synthetic_rt_world

N_FILES = 3
# fit_and_predict's launch (rt_model.hip): nb = min(256, max(1, ceil(n / 256))) blocks of xtx_kernel, per = ceil(n / nb) rows per
# block, embedded XTX_STAGE rows at a time; predict_kernel runs PRED_THREADS rows per block
XTX_MAX_BLOCKS, XTX_ROWS, XTX_STAGE, PRED_THREADS = 256, 256, 16, 64
SIZES = (255, 256, 257, 4097, 65536, 65537)

World = namedtuple("World", "name kind case n nb per train seams occupied clamps")
# case = (features, n_files, seq_off, seq, mono) as in rescore_edge_cases.RT_CASES; train: the training mask by construction;
# seams: name -> row index; occupied: the seam names that hold a training row; clamps: predictions must leave the range at both ends


def launch(n):
    nb = min(XTX_MAX_BLOCKS, max(1, -(-n // XTX_ROWS)))
    return nb, -(-n // nb)


def seams(n):
    """name -> row index of the places where a blocked, staged sum over n rows can lose or double a row."""
    nb, per = launch(n)
    last = (n - 1) // per  # the last block that holds a row
    lo, hi = last * per, min(last * per + per, n)
    s = {"first": 0, "stage_end": XTX_STAGE - 1, "stage_start": XTX_STAGE, "block_end": per - 1, "block_start": per,
         "block2_stage_end": per + XTX_STAGE - 1, "block2_stage_start": per + XTX_STAGE, "last_block_start": lo,
         "last_stage_start": lo + XTX_STAGE * ((hi - lo - 1) // XTX_STAGE), "last_block_hi-1": hi - 1, "n-1": n - 1,
         "predict_block_end": PRED_THREADS - 1, "predict_block_start": PRED_THREADS,
         "last_predict_block_start": PRED_THREADS * ((n - 1) // PRED_THREADS)}
    return {k: v for k, v in s.items() if 0 <= v < n}


def _arrange(train, want_train, want_other):
    """A permutation `src` (new row r is old row src[r]) with training rows at `want_train`, others at `want_other`, the rest in
    their old relative order."""
    n = len(train)
    want_train = sorted(set(want_train))
    want_other = sorted(set(want_other) - set(want_train))
    t, o = list(np.flatnonzero(train)), list(np.flatnonzero(~train))
    assert len(t) >= len(want_train) and len(o) >= len(want_other)
    src = np.full(n, -1, np.int64)
    src[want_train] = t[:len(want_train)]
    src[want_other] = o[:len(want_other)]
    rest = np.sort(np.array(t[len(want_train):] + o[len(want_other):], np.int64))
    src[src < 0] = rest
    assert np.array_equal(np.sort(src), np.arange(n))
    return src


def _rank(f, first, rng):
    """Rewrite `poisson` (the key of the q-value pass, ascending) so that the rows `first` come first, then every decoy, then the
    other targets: spectrum_q is 1 / len(first) on `first` and (1 + decoys) / targets or more after it."""
    n = len(f)
    decoy = f["label"] == -1
    rest_t = np.flatnonzero(~decoy & ~first)
    order = np.concatenate([rng.permutation(np.flatnonzero(first)), rng.permutation(np.flatnonzero(decoy)), rng.permutation(rest_t)])
    f["poisson"][order] = -0.5 * (n - np.arange(n))  # distinct, ascending along `order`
    assert first.sum() >= 100 and (1 + decoy.sum()) > 0.01 * (~decoy).sum()


def _sequences(kind, pep_len, rng):
    letters = np.frombuffer(_AA.encode(), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(pep_len)]).astype(np.int64)
    res = letters[rng.choice(len(_AA), size=int(off[-1]), p=_FREQ)]
    odd = rng.random(len(res)) < 0.04  # X, B: outside VALID_AA (they embed as index 0); U, O: its last two entries
    res[odd] = np.frombuffer(b"XBUO", dtype=np.uint8)[rng.integers(0, 4, int(odd.sum()))]
    return off, res


def _build(name, kind, n, seed, one_train=False, tail=0, mono_zero=False, keep_ims=False):
    rng = np.random.default_rng(seed)
    with np.errstate(invalid="ignore"):
        f, _, _, _ = synthetic_rt_world(n, N_FILES, seed=seed)
    target = f["label"] == 1
    m = max(100, n // 4)
    first = np.zeros(n, bool)
    first[np.flatnonzero(target)[np.argsort(f["poisson"][target], kind="stable")[:m]]] = True
    _rank(f, first, rng)
    train = first.copy()
    if one_train:  # label 0 is neither a decoy (label == -1) nor a training row (label == 1): 1 / m stays <= 0.01 with one row left
        keep = np.flatnonzero(first)[m // 2]
        f["label"][first] = 0
        f["label"][keep] = 1
        train[:] = False
        train[keep] = True

    # ---- peptides: sequences shared by the PSMs of a peptide key ----
    pep, inv = np.unique(f["peptide_idx"], return_inverse=True)
    n_pep = len(pep)
    pep_trains = np.zeros(n_pep, bool)
    pep_trains[inv[train]] = True
    lens = (1, 2, 3, 4) if kind == "rt" else (1, 2, 4, 8, 16, 32)
    pep_len = rng.integers(1, 41, n_pep) if kind == "rt" else rng.choice(lens, n_pep)
    tp = np.flatnonzero(pep_trains)
    if not one_train:  # every short length (the cterm branches of both embeddings) twice among the training peptides
        pep_len[tp[:2 * len(lens)]] = np.tile(lens, 2)
    long_len = 40 if kind == "rt" else 32
    # homopolymers whose predictions leave the clamp range (the laws below): F raises the retention and D lowers it, among
    # non-training peptides only (an observed retention cannot leave the run); W raises the mobility and G lowers it, among
    # training peptides too (im worlds: their ims leaves [0.5, 1.5] with the law)
    spare = np.flatnonzero(~pep_trains)
    homo_rt = spare[:8]
    homo_im = np.concatenate([tp[2 * len(lens):][:4], spare[8:12]]) if kind == "im" else spare[8:8]
    pep_len[homo_rt] = pep_len[homo_im] = long_len
    p_off, res = _sequences(kind, pep_len, rng)
    for group, pair in ((homo_rt, b"FD"), (homo_im, b"WG")):
        for j, p in enumerate(group):
            res[p_off[p]:p_off[p + 1]] = pair[j % 2]
    amap = np.zeros(256, np.int64)
    amap[np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYUO", dtype=np.uint8)] = np.arange(22)
    counts = np.zeros((n_pep, 22))
    np.add.at(counts, (np.repeat(np.arange(n_pep), pep_len), amap[res]), 1.0)
    is_homo = np.zeros(n_pep, bool)
    is_homo[homo_im] = True

    # ---- retention: linear in the composition, distorted per file (what global_alignment undoes), never near 0 ----
    h = rng.normal(0.0, 0.012, 22)
    h[amap[ord("F")]], h[amap[ord("D")]] = 0.05, -0.04
    rel_p = (0.5 + counts @ h).clip(0.06, 0.94)
    file_id = f["file_id"].astype(np.int64)
    slope, icpt, run_len = rng.uniform(0.8, 1.1, N_FILES), rng.uniform(0.0, 0.04, N_FILES), rng.uniform(55.0, 120.0, N_FILES)
    rel = np.where(train, rel_p[inv] + rng.normal(0, 0.005, n), rng.uniform(0.05, 0.95, n)).clip(0.05, 0.95)
    f["rt"] = (((rel - icpt[file_id]) / slope[file_id]).clip(0.02, 1.0) * run_len[file_id]).astype(np.float32)

    # ---- mobility: linear in composition and charge, on the 2^-10 grid; the bulk in [0.5, 1.5], homopolymers where the law puts them
    if kind == "im":
        f["charge"] = rng.choice([1, 2, 4], n)
        mono_p = np.zeros(n_pep) if mono_zero else rng.choice([1000.0, 2000.0, 3000.0, 4000.0], n_pep)
    else:
        mono_p = np.zeros(n_pep)
    w = rng.uniform(0.0, 1.0, 22)
    w[amap[ord("W")]], w[amap[ord("G")]] = 4.0, -2.0
    z = f["charge"].astype(np.float64)
    law = 0.625 + (counts @ w)[inv] / 64.0 + 0.125 * np.log2(z)
    ims = np.where(train | is_homo[inv], law + rng.normal(0, 0.01, n), rng.uniform(0.5, 1.5, n))
    ims = np.where(is_homo[inv], ims, ims.clip(0.5, 1.5))
    # rt worlds carry no ion mobility (ims == 0, the normal case without it): the mobility model's sums are not order-free there
    # (counts / length for lengths 1 .. 40), and with the two mass columns exactly zero the reference's ladder of regularisers
    # (gauss.rs:42-51: retry with 10 x eps until left_solved()) ends on another eps for another order of the same sums — measured
    # with seed 7051: eps 1e-8 for the sequential sums, 1.0 for the blocked ones, predictions 0.053 apart, both by the oracle's
    # own solve (LADDER_WORLD keeps the mobilities; tests/test_rt_model_cpu.py reproduces it).  With a zero target every eps
    # gives beta == 0.
    f["ims"] = (np.round(ims * 1024.0) / 1024.0).astype(np.float32) if kind == "im" or keep_ims else 0.0
    f["peptide_len"] = pep_len[inv]
    f["calcmass"] = mono_p[inv]

    # ---- training rows onto the seams ----
    sm = seams(n)
    if one_train:
        want_train, want_other = [sm["block_start"]], [v for k, v in sm.items() if k != "block_start"]
    elif tail:
        want_train = [v for v in sm.values() if v < n - tail]
        want_other = list(range(n - tail, n))
    else:
        want_train, want_other = list(sm.values()), []
    src = _arrange(train, want_train, want_other)
    f, inv, train = f[src], inv[src], train[src]
    f["spec_index"] = np.arange(n)
    row_len = pep_len[inv]
    seq_off = np.concatenate([[0], np.cumsum(row_len)]).astype(np.uint64)
    idx = np.repeat(p_off[:-1][inv] - seq_off[:-1].astype(np.int64), row_len) + np.arange(int(seq_off[-1]))
    nb, per = launch(n)
    occupied = tuple(k for k, v in sm.items() if train[v])
    return World(name, kind, (f, N_FILES, seq_off, res[idx].copy(), mono_p[inv].astype(np.float32)), n, nb, per, train, sm, occupied,
                 n >= 4097 and not one_train)


_SPECS = {}
for _k, _kind in enumerate(("rt", "im")):
    for _j, _n in enumerate(SIZES):
        _SPECS[f"{_kind}_exact/n{_n}"] = dict(kind=_kind, n=_n, seed=7000 + 100 * _k + _j)
    _SPECS[f"{_kind}_exact/one_train"] = dict(kind=_kind, n=600, seed=7050 + 100 * _k, one_train=True)
    _SPECS[f"{_kind}_exact/tail300"] = dict(kind=_kind, n=4097, seed=7051 + 100 * _k, tail=300)
_SPECS["rt_exact/n65537"]["seed"] = 7008  # (with 7005 the exactly singular X^T X fails the elimination: no retention model)
_SPECS["im_exact/n4097_mono0"] = dict(kind="im", n=4097, seed=7152, mono_zero=True)
WORLD_NAMES = tuple(_SPECS)
LADDER_WORLD = "rt_exact/tail300_with_ims"  # not among WORLD_NAMES: see the comment on ims in _build
_SPECS[LADDER_WORLD] = dict(_SPECS["rt_exact/tail300"], keep_ims=True)


@functools.lru_cache(maxsize=None)
def world(name):
    """The named world (built once per process; treat its arrays as read-only)."""
    return _build(name, **_SPECS[name])
