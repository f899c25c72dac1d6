"""A SECOND, independent reading of label-free quantification's integration stage — TEST INFRASTRUCTURE.

Written from the reference's Rust alone (crates/sage/src/lfq.rs: Traces::find_time_warps :361-385, apply_time_warps :388-400,
scores :402-437, integrate :447-509, Grid::summarize_traces :558-610, gaussian_kernel :614-628, convolve :632-646; fdr.rs:
picked_precursor :228-287), without consulting tests/lfq_reference.py or sage_amd/csrc/lfq.hip.  Where lfq_reference.py walks
bins, offsets and files one at a time, this file computes whole arrays: every bin of every row at once, all 151 offsets at
once, the bound walks as index searches.  tests/test_lfq_second_reading.py holds the two readings equal bit for bit.

The reference's addition orders are kept, because they decide the last bit:
  - convolve folds its <= 10 products from 0.0, left to right (:643);
  - a warp's dot product runs over i ascending and skips the terms whose j falls outside the run (:371-376) — skips, so a
    non-finite reference cell beside the edge never meets a padding zero;
  - the per-column sums over files start from 1.0 (summed_int) and 0.0 (weighted) (:407-412, :497-506);
  - Sum integration folds dot_product[file][left..right] from 0.0 (:488-490).
A masked term is added as +0.0: an accumulator that starts at +0.0 never becomes -0.0, so x + 0.0 == x bit for bit.

Transcendentals are the host libm's, one call per value (acos, pow, exp through `math`): numpy's own array versions may
differ from libm in the last bit, and f64::acos / powf / exp are libm's.

Input: the grid matrix [files * 3, 100] f64, the isotope distribution f32[3], the reference file and the settings
(peak_scoring, integration, spectral_angle as LfqSettings holds it).  Nothing is taken from the tracing pass."""
import math

import numpy as np

GRID = 100        # lfq.rs:21
N_ISO = 3         # lfq.rs:23
K_WIDTH = 10      # lfq.rs:17
SLACK = 75        # lfq.rs:350

_I = np.arange(GRID)


def kernel():
    """gaussian_kernel(0.5, K_WIDTH), lfq.rs:614-628"""
    sigma = 0.5
    step = 2.0 / (K_WIDTH - 1)
    constant = 1.0 / (sigma * math.sqrt(2.0 * math.pi))
    k = []
    for i in range(K_WIDTH):
        x = i * step - 1.0
        h = x / sigma
        k.append(constant * math.exp(-0.5 * (h * h)))
    total = 0.0
    for v in k:
        total += v
    return np.array([v / total for v in k])


_KERNEL = kernel()
# lfq.rs:634-641: n = len - len / 2; kernel[len.saturating_sub(n + idx)..] zipped with slice[idx.saturating_sub(n - 1)..]
_N = K_WIDTH - K_WIDTH // 2
_KS = np.maximum(K_WIDTH - (_N + _I), 0)[:, None] + np.arange(K_WIDTH)[None, :]       # [bin, term] kernel index
_WS = np.maximum(_I - (_N - 1), 0)[:, None] + np.arange(K_WIDTH)[None, :]             # [bin, term] signal index
_CONV_OK = (_KS < K_WIDTH) & (_WS < GRID)                                               # zip stops at the shorter one
_KS_C, _WS_C = np.minimum(_KS, K_WIDTH - 1), np.minimum(_WS, GRID - 1)
# lfq.rs:369-376: offsets -slack..=slack, j = i + offset
_OFF = np.arange(-SLACK, SLACK + 1)
_J = _OFF[:, None] + _I[None, :]                                                        # [offset, i]
_J_OK = (_J >= 0) & (_J < GRID)
_J_C = np.clip(_J, 0, GRID - 1)
# lfq.rs:418-431: (1 - |rt - center| / center).powf(0.33)
_CENTER = GRID // 2
_RT_BASE = [1.0 - (abs(rt - _CENTER) / _CENTER) for rt in range(GRID)]
_RT_POW = np.array([math.pow(b, 0.33) for b in _RT_BASE])


def convolve(rows):
    """convolve (lfq.rs:632-646) of every row and bin at once: [rows, GRID] -> [rows, GRID]"""
    rows = np.asarray(rows, dtype=np.float64)
    acc = np.zeros(rows.shape)
    with np.errstate(all="ignore"):
        for t in range(K_WIDTH):
            term = rows[:, _WS_C[:, t]] * _KERNEL[_KS_C[:, t]][None, :]
            acc = acc + np.where(_CONV_OK[:, t][None, :], term, 0.0)
    return acc


def _acos(x):
    flat = [math.acos(v) if -1.0 <= v <= 1.0 else math.nan for v in np.asarray(x, dtype=np.float64).ravel().tolist()]
    return np.array(flat).reshape(np.shape(x))


def summarize(matrix, dist):
    """Grid::summarize_traces (lfq.rs:558-610): (dot_product, spectral_angle), each [files, GRID]"""
    dist = np.asarray(dist, dtype=np.float32)
    total = np.float32(0.0)
    for d in dist:                       # .map(|x| x.powi(2)).sum::<f32>()
        total = total + d * d
    ss_dist = float(np.sqrt(total))      # f32 sqrt, then `as f64`
    conv = convolve(matrix)
    files = conv.shape[0] // N_ISO
    per_file = conv.reshape(files, N_ISO, GRID)
    dot = np.zeros((files, GRID))
    ss = np.zeros((files, GRID))
    with np.errstate(all="ignore"):
        for iso in range(N_ISO):
            dot = dot + per_file[:, iso, :] * float(dist[iso])
            ss = ss + per_file[:, iso, :] * per_file[:, iso, :]
        positive = ss > 0.0
        sim = np.where(positive, dot / (np.sqrt(ss) * ss_dist), 0.0)
        angle = 1.0 - 2.0 * _acos(sim) / math.pi
    return dot, angle


def find_time_warps(dot, ref):
    """Traces::find_time_warps (lfq.rs:361-385) for every file and offset at once"""
    files = dot.shape[0]
    reference = dot[ref]
    acc = np.zeros((files, len(_OFF)))
    with np.errstate(all="ignore"):
        for i in range(GRID):
            term = reference[i] * dot[:, _J_C[:, i]]                  # [files, offsets]
            acc = acc + np.where(_J_OK[:, i][None, :], term, 0.0)
    warps = []
    for row in acc:
        # `dot >= best.1` from (0, 0.0): the running best is the largest value that is >= 0.0, and the last offset that
        # reaches it stays; a NaN never compares
        with np.errstate(invalid="ignore"):
            cand = row >= 0.0
        if not cand.any():
            warps.append(0)
            continue
        top = row[cand].max()
        warps.append(int(_OFF[np.flatnonzero(cand & (row == top))[-1]]))
    return warps, acc


def apply_time_warps(mat, warps):
    """lfq.rs:388-400: shifted[i] = run[i + warp] inside the run, 0.0 outside"""
    j = _I[None, :] + np.asarray(warps)[:, None]
    ok = (j >= 0) & (j < GRID)
    return np.where(ok, np.take_along_axis(mat, np.clip(j, 0, GRID - 1), axis=1), 0.0)


def column_sums(dot, angle):
    """the fold over files of lfq.rs:407-412 for every column: (weighted / summed_int, summed_int)"""
    summed = np.full(dot.shape[1], 1.0)
    weighted = np.zeros(dot.shape[1])
    with np.errstate(all="ignore"):
        for f in range(dot.shape[0]):
            weighted = weighted + angle[f] * dot[f]
            summed = summed + dot[f]
        return weighted / summed, summed


def scores(dot, angle, strategy):
    """Traces::scores (lfq.rs:402-437)"""
    spectral, intensity = column_sums(dot, angle)
    top = float(np.fmax.reduce(intensity, initial=0.0))  # f64::max from 0.0: a NaN operand is dropped
    with np.errstate(all="ignore"):
        rel = np.sqrt(intensity / top)
        if strategy == "RetentionTime":
            sc = _RT_POW.copy()
        elif strategy == "SpectralAngle":
            sc = spectral.copy()
        elif strategy == "Intensity":
            sc = rel
        elif strategy == "Hybrid":
            sc = spectral * (spectral * spectral) * _RT_POW * rel   # s.powi(3) * rt.powf(0.33) * (i / max).sqrt()
        else:
            raise ValueError(strategy)
    return sc, spectral


def integrate(matrix, dist, ref, settings):
    """summarize_traces, then Traces::integrate (lfq.rs:447-509).  Returns a dict: warps, peak (has a peak), and with a peak
    rt, left, right, areas, score, spectral_angle; `dots` (the 151 warp dot products per file) for the tests' assertions."""
    matrix = np.asarray(matrix, dtype=np.float64)
    dot, angle = summarize(matrix, dist)
    warps, dots = find_time_warps(dot, ref)
    angle, dot = apply_time_warps(angle, warps), apply_time_warps(dot, warps)
    sc, spectral = scores(dot, angle, settings["peak_scoring"])
    thr = settings["spectral_angle"]
    with np.errstate(invalid="ignore"):
        passes = spectral >= thr
        # `*s > best.score && ..` from 0.0: the running best is the largest passing score above 0.0, the first bin that
        # reaches it stays
        eligible = (sc > 0.0) & passes
    if not eligible.any():               # best.score == 0.0
        return dict(peak=False, warps=warps, dots=dots)
    best = sc[eligible].max()
    rt = int(np.flatnonzero(eligible & (sc == best))[0])
    threshold = best * 0.50
    with np.errstate(invalid="ignore"):
        inside = np.concatenate([(sc >= threshold) & passes, [False]])   # a bound walk goes on while this holds
    idx = np.arange(GRID + 1)
    lmin = max(rt - GRID // 5, 0)
    start = max(rt - 1, 0)
    left = int(np.flatnonzero(((idx <= lmin) | ~inside) & (idx <= start))[-1])
    rmax = min(GRID - 1, rt + 20)
    right = int(np.flatnonzero(((idx >= rmax) | ~inside) & (idx >= rt + 1))[0])
    if settings["integration"] == "Sum":
        areas = np.zeros(dot.shape[0])
        with np.errstate(all="ignore"):
            for c in range(left, right):
                areas = areas + dot[:, c]
    elif settings["integration"] == "Apex":
        areas = dot[:, rt].copy()
    else:
        raise ValueError(settings["integration"])
    at_best, _ = column_sums(dot[:, rt:rt + 1], angle[:, rt:rt + 1])
    return dict(peak=True, warps=warps, dots=dots, rt=rt, left=left, right=right, areas=areas.tolist(), score=float(best),
                spectral_angle=float(at_best[0]))


def picked_precursor(decoy, score):
    """fdr::picked_precursor (fdr.rs:228-287) over rows in the caller's order (the reference's own row order is a hash map's;
    the sort is stable, so the caller's order is the tie order).  decoy: bool[n]; score: f64[n].  Returns (q f32[n], passing)."""
    decoy = np.asarray(decoy, dtype=bool)
    s = np.asarray(score, dtype=np.float64).astype(np.float32)           # peak.score as f32
    bits = s.view(np.uint32).astype(np.int64)
    key = np.where(bits >> 31, bits ^ 0xFFFFFFFF, bits ^ 0x80000000)     # f32::total_cmp as an ascending key
    order = np.argsort(-key, kind="stable")                                # b.score.total_cmp(&a.score)
    d = decoy[order]
    n_decoy = np.float32(1.0) + np.cumsum(d, dtype=np.float32)
    n_target = np.cumsum(~d, dtype=np.float32)
    with np.errstate(divide="ignore"):
        q = (n_decoy / n_target).astype(np.float32)
    q = np.minimum(np.float32(1.0), np.minimum.accumulate(q[::-1])[::-1]).astype(np.float32)
    passing = int(((q <= np.float32(0.05)) & ~d).sum())
    out = np.empty(len(s), np.float32)
    out[order] = q
    return out, passing
