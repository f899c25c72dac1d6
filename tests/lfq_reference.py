"""Sequential numpy / Python restatement of sage-core's label-free quantification (crates/sage/src/lfq.rs, isotopes.rs and
fdr::picked_precursor, fdr.rs:228-287) for MS1 spectra without ion mobility.  The checker of sage_hip_lfq.

Where the reference leaves an order open, this file fixes the one the device uses:
  - feature map: windows sorted by (rt, peptide, charge, isotope, decoy), then each 16 384-window page by (mass_lo, position in
    the rt order) — rt and mass_lo in f32 total order;
  - traces: every grid cell receives its additions in the order MS1 spectrum (as given: file order, then index in the file),
    peak (ascending mass, stable), match (page, then position inside the page);
  - grids and output rows: ascending (peptide, charge, decoy), charge 0 when charge states are combined;
  - picked_precursor: a stable sort by f32 score descending (f32 total order) of the rows in that order.
f32 arithmetic is done on np.float32 scalars (IEEE single, no contraction), f64 on Python floats."""
import math

import numpy as np

RT_TOL = np.float32(0.0050)
K_WIDTH = 10
GRID_SIZE = 100
N_ISOTOPES = 3
BIN_SIZE = 16 * 1024
NEUTRON = np.float32(1.00335)
PROTON = np.float32(1.0072764)
DECOY_SHIFT = np.float32(11.06)
SCORING = ("RetentionTime", "SpectralAngle", "Intensity", "Hybrid")
INTEGRATION = ("Apex", "Sum")

# mass.rs:78-104 composition(aa): (carbon, sulfur)
_COMPOSITION = {"A": (3, 0), "R": (6, 0), "N": (4, 0), "D": (4, 0), "C": (3, 1), "E": (5, 0), "Q": (5, 0), "G": (2, 0),
                "H": (6, 0), "I": (6, 0), "L": (6, 0), "K": (6, 0), "M": (5, 1), "F": (9, 0), "P": (5, 0), "S": (3, 0),
                "T": (4, 0), "W": (11, 0), "Y": (9, 0), "V": (5, 0), "U": (3, 0), "O": (12, 0)}

F32 = np.float32


def default_settings(**kw):
    """LfqSettings::default (lfq.rs:56-68)."""
    s = dict(peak_scoring="Hybrid", integration="Sum", spectral_angle=0.70, ppm_tolerance=5.0, mobility_pct_tolerance=1.0,
             combine_charge_states=True, peptide_q_value=0.01)
    s.update(kw)
    return s


def composition(sequence: str):
    c = s = 0
    for r in sequence:
        a, b = _COMPOSITION.get(r, (0, 0))
        c += a
        s += b
    return c, s


def _conv4(a, b):  # isotopes.rs:2-10, f32, left to right
    return [a[0] * b[0], a[0] * b[1] + a[1] * b[0], a[0] * b[2] + a[1] * b[1] + a[2] * b[0],
            a[0] * b[3] + a[1] * b[2] + a[2] * b[1] + a[3] * b[0]]


def _powi(x, k):  # f32::powi for k <= 3: x, x * x, x * (x * x)
    return [F32(1.0), x, x * x, x * (x * x)][k]


def _libm_expf():
    import ctypes
    import ctypes.util
    f = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").expf
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    return f


_EXPF = _libm_expf()


def _expf(x) -> np.float32:
    """f32::exp is libm expf (numpy's own float32 exp differs from it in the last bit for some inputs)"""
    return F32(_EXPF(float(x)))


def peptide_isotopes(carbons: int, sulfurs: int) -> np.ndarray:
    """isotopes.rs:43-50 (f32 throughout; exp is libm expf)."""
    fact = [1, 1, 2, 6]
    lam = F32(carbons) * F32(0.011)
    c13 = [_powi(lam, k) * _expf(-lam) / F32(fact[k]) for k in range(4)]
    l33, l35 = F32(sulfurs) * F32(0.0076), F32(sulfurs) * F32(0.044)
    s35 = [_powi(l35, 0) * _expf(-l35), F32(0.0), _powi(l35, 1) * _expf(-l35), F32(0.0)]
    s33 = [_powi(l33, k) * _expf(-l33) / F32(fact[k]) for k in range(4)]
    c = _conv4(c13, _conv4(s33, s35))
    mx = max(max(c[0], c[1]), c[2])
    return np.array([c[0] / mx, c[1] / mx, c[2] / mx], dtype=np.float32)


def total_key(x) -> int:
    """f32::total_cmp as an ascending unsigned key."""
    b = int(np.float32(x).view(np.uint32))
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def partition_point(keys, pred) -> int:
    lo, hi = 0, len(keys)
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(keys[mid]):
            lo = mid + 1
        else:
            hi = mid
    return lo


def search_keys(keys, lo_k: int, hi_k: int):
    """binary_search_slice (database.rs:549-561) over ascending integer keys: left index minus one, saturating."""
    left = max(partition_point(keys, lambda k: k < lo_k) - 1, 0)
    right = partition_point(keys[left:], lambda k: k <= hi_k) + left
    return left, right


def binary_search_slice(values, low, high):
    """binary_search_slice over f32 values compared with total_cmp."""
    return search_keys([total_key(v) for v in values], total_key(low), total_key(high))


def tol_bounds_ppm(center, ppm: float):
    """Tolerance::Ppm(-ppm, ppm).bounds (mass.rs:21-27), f32."""
    lo, hi = F32(-ppm), F32(ppm)
    return center + center * lo / F32(1000000.0), center + center * hi / F32(1000000.0)


def gaussian_kernel(sigma: float, n: int):
    """lfq.rs:592-608 (f64; exp is libm exp)."""
    step = 2.0 / (n - 1)
    const = 1.0 / (sigma * math.sqrt(2.0 * math.pi))
    k = []
    for i in range(n):
        x = i * step - 1.0
        q = x / sigma
        k.append(const * math.exp(-0.5 * (q * q)))
    s = 0.0
    for v in k:
        s += v
    return [v / s for v in k]


def convolve(sig, kernel) -> np.ndarray:
    """lfq.rs:612-627 for rows of a matrix at once: out[idx] = fold(0.0, + w[j] * k[j]) in j order, exactly as the loop."""
    sig = np.atleast_2d(np.asarray(sig, dtype=np.float64))
    kl, n = len(kernel), sig.shape[-1]
    mid = kl - kl // 2
    out = np.zeros_like(sig)
    for idx in range(n):
        ks, ws = max(kl - (mid + idx), 0), max(idx - (mid - 1), 0)
        acc = np.zeros(sig.shape[0])
        for j in range(min(kl - ks, n - ws)):
            acc = acc + sig[:, ws + j] * kernel[ks + j]
        out[:, idx] = acc
    return out


def select_features(feats: dict, settings: dict):
    """build_feature_map's first pass (lfq.rs:99-141): features in confidence order; the first one per peptide_idx with
    peptide_q <= peptide_q_value and label == 1.  Returned sorted by peptide_idx."""
    thr = F32(settings["peptide_q_value"])
    seen = {}
    for j in range(len(feats["peptide_idx"])):
        if F32(feats["peptide_q"][j]) <= thr and int(feats["label"][j]) == 1:
            p = int(feats["peptide_idx"][j])
            if p not in seen:
                seen[p] = (F32(feats["aligned_rt"][j]), F32(feats["calcmass"][j]), int(feats["file_id"][j]))
    return [(p,) + seen[p] for p in sorted(seen)]


def build_feature_map(settings: dict, precursor_charge, feats: dict):
    """lfq.rs:94-193 with the stated sort keys.  Returns a dict of per-window lists in final order, and min_rts."""
    sel = select_features(feats, settings)
    ppm = abs(float(settings["ppm_tolerance"]))
    rows = []
    for p, rt, calc, fid in sel:
        for z in range(precursor_charge[0], precursor_charge[1] + 1):
            for iso in range(N_ISOTOPES):
                mass = (calc + F32(iso) * NEUTRON) / F32(z)
                lo, hi = tol_bounds_ppm(mass, ppm)
                rows.append(dict(rt=rt, mass_lo=lo, mass_hi=hi, peptide=p, charge=z, isotope=iso, file_id=fid, decoy=False))
                lo, hi = tol_bounds_ppm(mass + DECOY_SHIFT, ppm)
                rows.append(dict(rt=max(rt - RT_TOL * F32(2.0), F32(0.0)), mass_lo=lo, mass_hi=hi, peptide=p, charge=z,
                                 isotope=iso, file_id=fid, decoy=True))
    # generation order is (peptide, charge, isotope, decoy): a stable sort by rt keeps it as the tie key
    rows = sorted(rows, key=lambda r: total_key(r["rt"]))
    min_rts = []
    for a in range(0, len(rows), BIN_SIZE):
        min_rts.append(rows[a]["rt"])
        rows[a:a + BIN_SIZE] = sorted(rows[a:a + BIN_SIZE], key=lambda r: total_key(r["mass_lo"]))
    return dict(ranges=rows, min_rts=min_rts, mass_keys=[total_key(r["mass_lo"]) for r in rows],
                rt_keys=[total_key(v) for v in min_rts])


def process_ms1(mz, intensity):
    """SpectrumProcessor::process for an MS1 spectrum without mobility (spectrum.rs:380-412): every peak as mz - PROTON,
    sorted stably by mass."""
    m = np.asarray(mz, dtype=np.float32) - PROTON
    order = sorted(range(len(m)), key=lambda i: total_key(m[i]))
    return m[order], np.asarray(intensity, dtype=np.float32)[order]


def spectrum_rt(sst, alignment) -> np.float32:
    _, max_rt, slope, intercept = alignment
    return (F32(sst) / F32(max_rt)) * F32(slope) + F32(intercept)


def mass_lookup(fmap, rt, mass):
    """FeatureMap::rt_slice + Query::mass_lookup (lfq.rs:195-215, 538-551): the matching windows in match order."""
    ranges, keys = fmap["ranges"], fmap["mass_keys"]
    page_lo, page_hi = search_keys(fmap["rt_keys"], total_key(rt - RT_TOL), total_key(rt + RT_TOL))
    min_rt, max_rt = rt - RT_TOL, rt + RT_TOL
    d = F32(0.1)
    for page in range(page_lo, page_hi):
        a = page * BIN_SIZE
        b = min(a + BIN_SIZE, len(ranges))
        il, ir = search_keys(keys[a:b], total_key(mass - d), total_key(mass + d))
        for e in ranges[a + il:a + ir]:
            if e["rt"] <= max_rt and e["rt"] >= min_rt and mass >= e["mass_lo"] and mass <= e["mass_hi"]:
                yield e


def grid_key(e, combine: bool):
    return (e["peptide"], 0 if combine else e["charge"], bool(e["decoy"]))


def add_entry(grid, spectrum_rt_, isotope, file_id, intensity):
    """Grid::add_entry (lfq.rs:649-663)."""
    rt_min, rt_step, m = grid["rt_min"], grid["rt_step"], grid["matrix"]
    cols = m.shape[1]
    f = np.floor((spectrum_rt_ - rt_min) / rt_step)
    bin_lo = 0 if not (f > 0) else (cols - 1 if f >= cols - 1 else int(f))  # `as usize` saturates, NaN -> 0
    bin_hi = min(bin_lo + 1, cols - 1)
    bin_lo_rt = F32(bin_lo) * rt_step + rt_min
    interp = (spectrum_rt_ - bin_lo_rt) / rt_step
    row = file_id * N_ISOTOPES + isotope
    m[row, bin_lo] += float((F32(1.0) - interp) * intensity)
    m[row, bin_hi] += float(interp * intensity)


def trace(fmap, spectra, alignments, n_files: int, combine: bool, isotopes_of):
    """FeatureMap::quantify's tracing pass.  spectra: iterable of (file_id, scan_start_time, masses, intensities) of
    processed MS1 spectra in order; isotopes_of(peptide) -> f32[3].  Returns {key: grid}."""
    grids = {}
    step = (RT_TOL * F32(2.0)) / F32(GRID_SIZE)
    for file_id, sst, masses, ints in spectra:
        rt = spectrum_rt(sst, alignments[file_id])
        for mass, inten in zip(masses, ints):
            for e in mass_lookup(fmap, rt, F32(mass)):
                k = grid_key(e, combine)
                g = grids.get(k)
                if g is None:
                    g = grids[k] = dict(rt_min=e["rt"] - RT_TOL, rt_step=step, ref=e["file_id"],
                                        dist=isotopes_of(e["peptide"]),
                                        matrix=np.zeros((n_files * N_ISOTOPES, GRID_SIZE), dtype=np.float64))
                add_entry(g, rt, e["isotope"], file_id, F32(inten))
    return grids


def _seq_sum(a, axis=-1):
    """left-to-right f64 sum (np.cumsum accumulates sequentially)."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis))
    with np.errstate(invalid="ignore", over="ignore"):  # (inf - inf among the terms is a NaN sum, not an error)
        return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


_acos = np.vectorize(lambda x: math.acos(x) if -1.0 <= x <= 1.0 else math.nan, otypes=[np.float64])  # libm acos


def summarize(grid, kernel):
    """Grid::summarize_traces (lfq.rs:669-722): (dot_product, spectral_angle) of shape [files, GRID_SIZE]."""
    m, dist = grid["matrix"], grid["dist"]
    files = m.shape[0] // N_ISOTOPES
    ss_dist = float(np.sqrt(F32(F32(dist[0] * dist[0]) + F32(dist[1] * dist[1])) + F32(dist[2] * dist[2])))
    conv = convolve(m, kernel)
    dot = np.zeros((files, GRID_SIZE))
    ss = np.zeros((files, GRID_SIZE))
    for iso in range(N_ISOTOPES):
        c = conv[iso::N_ISOTOPES]
        dot = dot + c * float(dist[iso])
        ss = ss + c * c
    with np.errstate(divide="ignore", invalid="ignore"):
        sim = np.where(ss > 0.0, dot / (np.sqrt(ss) * ss_dist), 0.0)
        angle = 1.0 - 2.0 * _acos(sim) / math.pi
    return dot, angle


def warp_dots(dot, ref: int, slack: int = 75):
    """the dot product of every file with the reference file at every offset -slack..=slack: [files, 2 * slack + 1]"""
    n = dot.shape[1]
    reference = dot[ref]
    offs = np.arange(-slack, slack + 1)
    j = offs[:, None] + np.arange(n)[None, :]
    inside = (j >= 0) & (j < n)
    out = []
    for row in range(dot.shape[0]):
        with np.errstate(invalid="ignore", over="ignore"):
            prods = reference[None, :] * dot[row][np.clip(j, 0, n - 1)]
        # out-of-range terms are skipped by the reference (so a non-finite reference cell never meets a padding zero);
        # adding +0.0 in their place to a sum that is never -0.0 changes nothing
        out.append(_seq_sum(np.where(inside, prods, 0.0), axis=1))
    return np.array(out)


def find_time_warps(dot, ref: int, slack: int = 75):
    """Traces::find_time_warps (lfq.rs:386-411): `>=` keeps the last best offset."""
    warps = []
    for dots in warp_dots(dot, ref, slack):
        best_off, best = 0, 0.0
        for o, d in zip(range(-slack, slack + 1), dots.tolist()):
            if d >= best:
                best_off, best = o, d
        warps.append(best_off)
    return warps


def apply_time_warps(mat, warps):
    out = np.zeros_like(mat)
    n = mat.shape[1]
    for row, w in enumerate(warps):
        for i in range(n):
            j = i + w
            if 0 <= j < n:
                out[row, i] = mat[row, j]
    return out


def _div(a, b) -> float:
    """f64 division as IEEE 754 defines it (Python's own raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(x) -> float:
    """f64::sqrt: NaN for a negative or NaN operand (math.sqrt raises)"""
    return math.sqrt(x) if x >= 0.0 else math.nan


def rt_factor_table():
    """(1 - |rt - center| / center).powf(0.33) for the GRID_SIZE bins (libm pow)."""
    c = GRID_SIZE // 2
    return [math.pow(1.0 - (abs(rt - c) / c), 0.33) for rt in range(GRID_SIZE)]


def scores(dot, angle, strategy: str):
    """Traces::scores (lfq.rs:427-467)."""
    files, cols = dot.shape
    spectral, intensity = [], []
    mx = 0.0
    for col in range(cols):
        summed, weighted = 1.0, 0.0
        for f in range(files):
            weighted += angle[f, col] * dot[f, col]
            summed += dot[f, col]
        spectral.append(_div(weighted, summed))
        intensity.append(summed)
        mx = max(mx, summed)  # f64::max drops a NaN operand; so does this (mx is never NaN, and `nan > mx` is False)
    rtf = rt_factor_table()
    out = []
    for rt, (s, i) in enumerate(zip(spectral, intensity)):
        if strategy == "RetentionTime":
            out.append(rtf[rt])
        elif strategy == "SpectralAngle":
            out.append(s)
        elif strategy == "Intensity":
            out.append(_sqrt(_div(i, mx)))
        else:
            out.append(s * (s * s) * rtf[rt] * _sqrt(_div(i, mx)))
    return out, spectral


def integrate(grid, settings, kernel=None):
    """summarize_traces + Traces::integrate (lfq.rs:477-538).  None when no bin qualifies; else a dict with the peak and the
    intermediate results the device reports (warps, left / right bounds)."""
    kernel = kernel or gaussian_kernel(0.5, K_WIDTH)
    dot, angle = summarize(grid, kernel)
    warps = find_time_warps(dot, grid["ref"])
    angle, dot = apply_time_warps(angle, warps), apply_time_warps(dot, warps)
    sc, spectral = scores(dot, angle, settings["peak_scoring"])
    thr_sa = abs(float(settings["spectral_angle"]))
    best_rt, best = 0, 0.0
    for rt, s in enumerate(sc):
        if s > best and spectral[rt] >= thr_sa:
            best, best_rt = s, rt
    if best == 0.0:
        return dict(peak=False, warps=warps)
    left, right = max(best_rt - 1, 0), best_rt + 1
    threshold = best * 0.50
    n = len(sc)
    while left > max(best_rt - n // 5, 0) and sc[left] >= threshold and spectral[left] >= thr_sa:
        left -= 1
    while right < min(max(n - 1, 0), best_rt + 20) and sc[right] >= threshold and spectral[right] >= thr_sa:
        right += 1
    areas = []
    for f in range(dot.shape[0]):
        if settings["integration"] == "Sum":
            a = 0.0
            for v in dot[f, left:right]:
                a += v
            areas.append(a)
        else:
            areas.append(float(dot[f, best_rt]))
    summed, weighted = 1.0, 0.0
    for f in range(dot.shape[0]):
        weighted += angle[f, best_rt] * dot[f, best_rt]
        summed += dot[f, best_rt]
    return dict(peak=True, warps=warps, rt=best_rt, score=best, spectral_angle=_div(weighted, summed), areas=areas, left=left,
                right=right)


def picked_precursor(rows):
    """fdr.rs:228-287.  rows: [(key, score f64)] in ascending key order (key[-1] = decoy).  Returns ({key: q f32}, passing)."""
    order = sorted(range(len(rows)), key=lambda i: -total_key(F32(rows[i][1])))
    decoy, target = F32(1.0), F32(0.0)
    q = [F32(1.0)] * len(order)
    for j, i in enumerate(order):
        if rows[i][0][-1]:
            decoy += F32(1.0)
        else:
            target += F32(1.0)
        with np.errstate(divide="ignore"):
            q[j] = decoy / target
    q_min, passing = F32(1.0), 0
    for j in range(len(order) - 1, -1, -1):
        q_min = min(q_min, q[j])
        q[j] = q_min
        if q_min <= F32(0.05) and not rows[order[j]][0][-1]:
            passing += 1
    return {rows[i][0]: q[j] for j, i in enumerate(order)}, passing


def quantify(settings, precursor_charge, feats, spectra, alignments, n_files, isotopes_of, grids=None):
    """The whole LFQ block of runner.rs:562-575.  Returns (results {key: dict}, passing, grids)."""
    if grids is None:
        fmap = build_feature_map(settings, precursor_charge, feats)
        grids = trace(fmap, spectra, alignments, n_files, settings["combine_charge_states"], isotopes_of)
    kernel = gaussian_kernel(0.5, K_WIDTH)
    res = {k: integrate(grids[k], settings, kernel) for k in sorted(grids)}
    peaks = [(k, r["score"]) for k, r in res.items() if r["peak"]]
    q, passing = picked_precursor(peaks)
    for k, v in q.items():
        res[k]["q_value"] = v
    return res, passing, grids
