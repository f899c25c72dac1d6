"""A second reading of the predict_rt block (sage-cli runner.rs:513-530) in numpy and Python integers, written from the
reference's ml/qvalue.rs, ml/retention_alignment.rs, ml/retention_model.rs, ml/mobility_model.rs and ml/regression.rs.  It shares
nothing with linreg_fit / rt_embed / im_embed of oracle/rescore_oracle.cpp or with sage_amd/csrc/rt_model.hip, except the
Gauss-Jordan solve, which it takes from the oracle (oracle_lib.gauss_solve, held to gauss.rs by tests/test_rescore_oracle.py).

It is for the order-free worlds of tests/rt_model_worlds.py: X^T X, X^T y, sum y, sum y^2 and the count are accumulated as exact
integers on the world's dyadic grid and converted to f64 ONCE — which equals the reference's sequential f64 sums only while
those are exact (tests/test_rt_model_cpu.py asserts the budget).  predict() raises where a model's inputs leave the grid.
"""
import numpy as np

import oracle_lib

VALID_AA = b"ACDEFGHIKLMNPQRSTVWYUO"  # mass.rs:59-62
N_AA = len(VALID_AA)
RT_D, IM_D = N_AA * 3 + 3, N_AA * 4 + 12
AA_MAP = np.zeros(26, np.int64)  # retention_model.rs:64-67: letters outside VALID_AA keep index 0
AA_MAP[np.frombuffer(VALID_AA, dtype=np.uint8) - ord("A")] = np.arange(N_AA)
# mobility_model.rs:39-73: letter offsets (b'L' - b'A', ...), compared with the residue's VALID_AA index as written (:113-132)
_o = lambda s: [c - ord("A") for c in s]  # noqa: E731
IM_CLASSES = {IM_D - 9: _o(b"LVIFWY"), IM_D - 10: _o(b"STNQ"), IM_D - 8: _o(b"RKH"), IM_D - 7: _o(b"DE"), IM_D - 11: _o(b"GAS"),
              IM_D - 12: _o(b"LIV")}


def _residues(seq_off, seq):
    off = np.asarray(seq_off, dtype=np.int64)
    lens = np.diff(off)
    row = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(int(off[-1])) - np.repeat(off[:-1], lens)
    idx = AA_MAP[np.asarray(seq, dtype=np.int64)[off[0]:off[-1]] - ord("A")]
    cterm = np.repeat(np.maximum(lens - 3, 0), lens)  # len.saturating_sub(3)
    return lens, row, pos, idx, cterm


def rt_embed(seq_off, seq, mono):
    """RetentionModel::embed (retention_model.rs:42-59) of every peptide: n x 69"""
    lens, row, pos, idx, cterm = _residues(seq_off, seq)
    e = np.zeros((len(lens), RT_D))
    np.add.at(e, (row, idx), 1.0)
    nterm = pos <= 1  # match aa_idx { 0 | 1 => N, x if x == cterm || x == cterm + 1 => C, _ => {} }: the first arm wins
    np.add.at(e, (row[nterm], N_AA + idx[nterm]), 1.0)
    ct = ~nterm & ((pos == cterm) | (pos == cterm + 1))
    np.add.at(e, (row[ct], 2 * N_AA + idx[ct]), 1.0)
    e[:, RT_D - 3] = lens
    e[:, RT_D - 2] = np.log1p(np.asarray(mono, dtype=np.float32).astype(np.float64))
    e[:, RT_D - 1] = 1.0
    return e


def im_embed(seq_off, seq, mono, charge):
    """MobilityModel::embed (mobility_model.rs:97-149) of every peptide: n x 100"""
    lens, row, pos, idx, cterm = _residues(seq_off, seq)
    e = np.zeros((len(lens), IM_D))
    np.add.at(e, (row, idx), 1.0)
    nterm = pos <= 1
    np.add.at(e, (row[nterm], 2 * N_AA + idx[nterm]), 1.0)
    ct = ~nterm & (pos > cterm)
    np.add.at(e, (row[ct], 3 * N_AA + idx[ct]), 1.0)
    for col, members in IM_CLASSES.items():
        hit = np.isin(idx, members)
        np.add.at(e, (row[hit], np.full(int(hit.sum()), col)), 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        e[:, N_AA:2 * N_AA] = e[:, :N_AA] / lens[:, None].astype(np.float64)
        z = np.asarray(charge).astype(np.float64)
        m = np.asarray(mono, dtype=np.float32).astype(np.float64)
        e[:, IM_D - 5] = z
        e[:, IM_D - 6] = 1.0 / z
        e[:, IM_D - 3] = lens
        e[:, IM_D - 2] = m / 1000.0
        e[:, IM_D - 4] = (m / z) / 1000.0
    e[:, IM_D - 1] = 1.0
    return e


def to_grid(a, bits):
    """a * 2^bits as int64; raises unless that is exact (every entry a multiple of 2^-bits, below 2^62)."""
    s = np.asarray(a, dtype=np.float64) * float(2 ** bits)  # a power-of-two scaling: exact
    if not (np.all(np.isfinite(s)) and np.all(s == np.rint(s)) and np.all(np.abs(s) < 2.0 ** 62)):
        raise ValueError(f"not on the 2^-{bits} grid")
    return s.astype(np.int64)


def _f64(k, bits):
    """The Python integer k, times 2^-bits, as the nearest f64 (one rounding; none while |k| < 2^53)."""
    return float(np.ldexp(float(int(k)), -bits))


def exact_sums(x, y, keep, x_bits, y_bits):
    """regression.rs:38-51 over the rows with keep: (X^T X [D, D], X^T y [D], sum y, sum y^2, count) as f64 converted once from
    integer sums, and the budget: the largest sum of |terms| of any entry of X^T X / X^T y, in units of its grid."""
    xi = to_grid(x[keep], x_bits)
    yi = to_grid(y[keep], y_bits)
    if len(yi) == 0:
        return None, None, 0.0, 0.0, 0, 0
    ax, ay = np.abs(xi), np.abs(yi)
    if int(ax.max()) * max(int(ax.max()), int(ay.max())) * len(yi) >= 2 ** 62:  # (Python integers) no int64 sum below can wrap
        raise ValueError("sums leave int64")
    budget = max(int((ax.T @ ax).max()), int((ax.T @ ay).max()))
    cov = (xi.T @ xi).astype(np.float64) * 2.0 ** (-2 * x_bits) if budget < 2 ** 53 else None
    b = (xi.T @ yi).astype(np.float64) * 2.0 ** (-(x_bits + y_bits)) if budget < 2 ** 53 else None
    sum_y = _f64(sum(int(v) for v in yi), y_bits)
    sum_y2 = _f64(sum(int(v) * int(v) for v in yi), 2 * y_bits)
    return cov, b, sum_y, sum_y2, len(yi), budget


def linreg(x, y, keep, x_bits, y_bits):
    """LinearRegression::fit (regression.rs:72-117) -> (beta, r2, budget) or (None, 0.0, budget)"""
    cov, b, sum_y, sum_y2, cnt, budget = exact_sums(x, y, keep, x_bits, y_bits)
    if cnt == 0:
        return None, 0.0, budget
    if cov is None:
        raise ValueError("the sums are not exact in f64: over 2^53 units")
    nf = float(cnt)
    y_mean = sum_y / nf
    y_var = sum_y2 - nf * y_mean * y_mean
    beta = oracle_lib.gauss_solve(cov, b)
    if beta is None:
        return None, 0.0, budget
    sse = 0.0
    for v in (dot_left_to_right(x[keep], beta) - y[keep]) ** 2:  # (pred - act).powi(2), summed in row order
        sse += float(v)
    with np.errstate(invalid="ignore", divide="ignore"):
        r2 = float(1.0 - np.float64(sse) / np.float64(y_var))
    return beta, r2, budget


def dot_left_to_right(x, beta):
    """fold(0.0, |sum, (x, w)| sum + x * w) per row (retention_model.rs:85-89): one rounded product, one rounded add per column"""
    pred = np.zeros(len(x))
    for j in range(x.shape[1]):
        pred = pred + x[:, j] * beta[j]
    return pred


def bounded(pred, observed, hi):
    """rt.clamp(0.0, hi) as f32 and (observed - bounded).abs() in f32 (retention_model.rs:19-22, mobility_model.rs:25-29)"""
    b = np.clip(pred, 0.0, hi).astype(np.float32)  # (a NaN stays a NaN, as in f64::clamp)
    return b, np.abs(np.asarray(observed, dtype=np.float32) - b)


# ---- ml/qvalue.rs and ml/retention_alignment.rs --------------------------------------------------------------------------------
def spectrum_q(poisson, label):
    """runner.rs:517-520: sort by poisson (f64 total order, stable), spectrum_q_value (qvalue.rs:8-36); input order"""
    bits = np.ascontiguousarray(poisson, dtype=np.float64).view(np.int64)
    order = np.argsort(np.where(bits < 0, bits ^ np.int64(0x7FFFFFFFFFFFFFFF), bits), kind="stable")
    d = (np.asarray(label) == -1)[order]
    with np.errstate(divide="ignore"):
        q = (1 + np.cumsum(d)).astype(np.float32) / np.cumsum(~d).astype(np.float32)
    q = np.minimum(np.minimum.accumulate(q[::-1])[::-1], np.float32(1.0))
    out = np.empty(len(q), np.float32)
    out[order] = q
    return out


def _f64_min(a, b):
    """f64::min: a NaN operand is ignored"""
    return b if a != a else (a if b != b else min(a, b))


def _ceil_as_u32(rt):
    c = np.ceil(np.asarray(rt, dtype=np.float32)).astype(np.float64)
    return np.where(np.isnan(c) | (c <= 0), 0.0, np.minimum(c, 4294967295.0))  # `as u32` saturates; NaN -> 0


def global_alignment(f, n_files, train):
    """retention_alignment.rs:95-173 -> (alignments [n_files, 3] f32 = max_rt, slope, intercept; aligned_rt f32).  Matrix rows in
    ascending peptide order, every sum sequential from its written start value (the order of oracle/rescore_oracle.cpp's header)."""
    file_id = f["file_id"].astype(np.int64)
    max_rt = np.zeros(n_files)
    np.maximum.at(max_rt, file_id, _ceil_as_u32(f["rt"]))
    rows = {}
    for i in np.flatnonzero(train):  # mean_rt_by_file: the minimum rt per (peptide, file)
        v = rows.setdefault(int(f["peptide_idx"][i]), {})
        k, rt = int(file_id[i]), float(f["rt"][i])
        v[k] = _f64_min(v[k], rt) if k in v else rt
    mat, mean_rts = [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for p in sorted(rows):
            v = np.full(n_files, np.nan)
            s, ln = 0.0, 0.0
            for k in sorted(rows[p]):
                v[k] = np.float64(rows[p][k]) / np.float64(max_rt[k])
                s, ln = s + v[k], ln + 1.0
            mean = np.float64(s) / np.float64(ln)
            if not (np.isfinite(mean) and abs(mean) >= np.finfo(np.float64).tiny):  # f64::is_normal
                continue
            fin = [x for x in v if np.isfinite(x)]
            s2 = 0.0
            for x in fin:
                s2 += x
            mat.append(v)
            mean_rts.append(np.float64(s2) / np.float64(len(fin)))
        al = np.zeros((n_files, 3), np.float32)
        for k in range(n_files):
            ln, dot, sx, sy = 0, 0.0, 0.0, 0.0
            xs = []
            for v, y in zip(mat, mean_rts):
                x = float(v[k])
                if not np.isfinite(x):
                    continue
                ln, dot, sx, sy = ln + 1, dot + x * float(y), sx + x, sy + float(y)
                xs.append(x)
            x_mean, y_mean = np.float64(sx) / np.float64(ln), np.float64(sy) / np.float64(ln)
            ssxy = np.float64(dot) - np.float64(ln) * x_mean * y_mean
            sx2 = np.float64(1e-8)
            for x in xs:
                sx2 = sx2 + (x - x_mean) * (x - x_mean)
            slope = ssxy / sx2
            icpt = y_mean - slope * x_mean
            slope = slope if np.isfinite(slope) else 1.0
            icpt = icpt if np.isfinite(icpt) else 0.0
            al[k] = (max_rt[k], slope, icpt)
        aligned = (f["rt"].astype(np.float32) / al[file_id, 0]) * al[file_id, 1] + al[file_id, 2]  # f32 throughout
    return al, aligned.astype(np.float32)


def predict(f, n_files, seq_off, seq, mono, exact):
    """The whole block.  `exact` names the model whose sums must be order-free: "rt" (design 2^0, target 2^-29) or "im" (design
    2^-5, target 2^-10).  The other model is not read here: its sums depend on the order.  Returns spectrum_q, train, alignments,
    aligned_rt, and of the exact model predicted, delta, fitted, r2, beta, budget, design and target."""
    q = spectrum_q(f["poisson"], f["label"])
    train = (f["label"] == 1) & (q <= np.float32(0.01))
    al, aligned = global_alignment(f, n_files, train)
    out = dict(spectrum_q=q, train=train, alignments=al, aligned_rt=aligned)
    if exact == "rt":
        x, y, hi, bits = rt_embed(seq_off, seq, mono), aligned.astype(np.float64), 1.0, (0, 29)
        observed = aligned
    else:
        x, y, hi, bits = im_embed(seq_off, seq, mono, f["charge"]), f["ims"].astype(np.float64), 2.0, (5, 10)
        observed = f["ims"]
    beta, r2, budget = linreg(x, y, train, *bits)
    n = len(f)
    if beta is None:  # Feature defaults, scoring.rs:576-592
        pred, delta = np.zeros(n, np.float32), np.full(n, 0.999, np.float32)
    else:
        pred, delta = bounded(dot_left_to_right(x, beta), observed, hi)
    out.update(predicted=pred, delta=delta, fitted=beta is not None, r2=r2, budget=budget, beta=beta, design=x, target=y)
    return out


_readings = {}


def readings(name):
    """(world, oracle_lib.predict_rt of it, predict() of it) of a world of tests/rt_model_worlds.py, computed once per process and
    shared by every test that needs them (treat as read-only)."""
    if name not in _readings:
        import rt_model_worlds
        w = rt_model_worlds.world(name)
        with np.errstate(invalid="ignore", divide="ignore"):
            _readings[name] = (w, oracle_lib.predict_rt(*w.case), predict(*w.case, exact=w.kind))
    return _readings[name]


def model_fields(kind):
    """(predicted, delta, index into the oracle's fitted / r2) of the model a world of `kind` makes order-free"""
    return ("predicted_rt", "delta_rt_model", 0) if kind == "rt" else ("predicted_ims", "delta_ims_model", 1)
