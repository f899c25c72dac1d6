"""A layout-free reading of label-free quantification's TRACING stage — TEST INFRASTRUCTURE, no test.

Written from the reference's Rust alone (crates/sage/src/lfq.rs: build_feature_map :94-170, quantify :239-286, Grid::new
:513-535, Grid::add_entry :538-550, Query::mass_lookup :649-675, mass_mobility_lookup :677-686; mass.rs: Tolerance::bounds
:21-35; spectrum.rs: the MS1 branches of SpectrumProcessor::process :344-412; database.rs: binary_search_slice :549-561),
without consulting tests/lfq_reference.py, tests/lfq_im_reference.py or sage_amd/csrc/lfq.hip.  It knows no page, no sort of
the windows and no binary search: every (peak, window) pair of a spectrum is put to the predicates of the final filter
(lfq.rs:668-673, :682-685) and nothing else.  (match_pruned forms fewer pairs, by one global search that step 3 below
justifies; it is held equal to the exhaustive match() on every world it is used on.)

Why that is the whole truth on some maps.  Call a map layout-free when every window has f32(mass_hi - 0.1f) <= mass_lo, no
window rt is NaN or -0.0 (so total_cmp is <=).  Let a window W in page k pass the four predicates for (rt, mass), with
low = rt - RT_TOL, high = rt + RT_TOL as f32 (lfq.rs:209-210, :218-219: the very values the predicates use).
  1. rt_slice (lfq.rs:205-221 over database.rs:549-561): page_hi counts the pages with min_rt <= high, and
     min_rts[k] <= W.rt <= high, so k < page_hi.  page_lo = P - 1 where P counts the pages with min_rt < low; if k < P - 1
     then min_rts[k + 1] < low and every window of page k, sorted by rt before the cut, has rt <= min_rts[k + 1] < low —
     but W.rt >= low.  So page_lo <= k: W's page is searched wherever the sort put W among equal rts.
  2. inside the page (lfq.rs:660-665), sorted by mass_lo: inner_right counts the windows with mass_lo <= f32(mass + 0.1),
     and W.mass_lo <= mass <= f32(mass + 0.1): W lies left of inner_right.
  3. inner_left is at most the count of windows with mass_lo < f32(mass - 0.1).  mass <= W.mass_hi and rounding is monotone,
     so f32(mass - 0.1) <= f32(W.mass_hi - 0.1) <= W.mass_lo: W is not among those, it lies at or right of inner_left.
Conversely the lookup yields nothing the filter rejects.  So on a layout-free map the set of (peak, window) matches is the set
of pairs that pass the predicates, whatever the sort did.  (Without the condition of 3. a window is found or missed by the
minus-one of database.rs:555 alone: that is the layout-dependent +-0.1 miss, and this module refuses such maps.)

The order of additions.  The reference's spectra run in parallel; the port adds in the order given: spectra as the batches
give them, a spectrum's peaks by ascending mass (stable), and add_entry's lower bin before its upper bin.  If no peak matches
two windows of one (grid, file, isotope) row — this module raises otherwise — every cell's additions are ordered by
(spectrum, peak) alone, and a left-to-right f64 fold per cell defines every grid bit for bit.

Everything is whole f32 arrays, each operation rounded once, in the reference's operation order."""
import numpy as np

F32 = np.float32
RT_TOL = F32(0.0050)           # lfq.rs:15
GRID_SIZE = 100                # lfq.rs:21
N_ISOTOPES = 3                 # lfq.rs:23
NEUTRON = F32(1.00335)         # mass.rs:7
PROTON = F32(1.0072764)        # mass.rs:6
DECOY_SHIFT = F32(11.06)       # lfq.rs:156
PRE_FILTER = F32(0.1)          # lfq.rs:663-664
MILLION = F32(1_000_000.0)     # mass.rs:24
HUNDRED = F32(100.0)           # mass.rs:29


class NotLayoutFree(ValueError):
    pass


def select(peptide_idx, label, peptide_q, threshold):
    """rows of the selected features, in confidence order (lfq.rs:100-105: the first passing row of every peptide)"""
    ok = np.flatnonzero((np.asarray(peptide_q, F32) <= F32(threshold)) & (np.asarray(label) == 1))
    _, first = np.unique(np.asarray(peptide_idx)[ok], return_index=True)
    return ok[np.sort(first)]


def _bounds(center, lo, hi, scale):
    """Tolerance::Ppm / Pct(lo, hi).bounds(center), mass.rs:23-32: center * lo / scale, then center + delta"""
    return center + (center * F32(lo)) / scale, center + (center * F32(hi)) / scale


def build_windows(peptide_idx, label, calcmass, aligned_rt, peptide_q, precursor_charge, ppm, peptide_q_value=0.01, ims=None,
                  mobility_pct=1.0):
    """The windows of lfq.rs:135-169 in generation order — feature (confidence order), charge, isotope, forward then decoy —
    as a dict of arrays; `feature` is the row of the feature table.  No sort."""
    rows = select(peptide_idx, label, peptide_q, peptide_q_value)
    charges = np.arange(int(precursor_charge[0]), int(precursor_charge[1]) + 1)
    shape = (len(rows), len(charges), N_ISOTOPES, 2)
    feat = np.broadcast_to(rows[:, None, None, None], shape)
    z = np.broadcast_to(charges[None, :, None, None], shape)
    iso = np.broadcast_to(np.arange(N_ISOTOPES)[None, None, :, None], shape)
    decoy = np.broadcast_to(np.array([False, True])[None, None, None, :], shape)
    cm = np.asarray(calcmass, F32)[feat]
    mass = (cm + iso.astype(F32) * NEUTRON) / z.astype(F32)                       # :140
    center = np.where(decoy, mass + DECOY_SHIFT, mass).astype(F32)                 # :156
    lo, hi = _bounds(center, -F32(ppm), F32(ppm), MILLION)
    frt = np.asarray(aligned_rt, F32)[feat]
    rt = np.where(decoy, np.maximum(frt - RT_TOL * F32(2.0), F32(0.0)), frt).astype(F32)   # :159
    w = dict(feature=feat, peptide=np.asarray(peptide_idx)[feat].astype(np.int64), charge=z.astype(np.int64), isotope=iso.astype(np.int64),
             decoy=decoy.copy(), rt=rt, mass_lo=lo.astype(F32), mass_hi=hi.astype(F32))
    if ims is not None:
        m = np.asarray(ims, F32)[feat]
        mlo, mhi = _bounds(m, -F32(mobility_pct), F32(mobility_pct), HUNDRED)     # :111-115
        w["mobility_lo"], w["mobility_hi"] = mlo.astype(F32), mhi.astype(F32)
    return {k: np.ascontiguousarray(v.reshape(-1)) for k, v in w.items()}


def require_layout_free(w):
    """raises unless every window has f32(mass_hi - 0.1f) <= mass_lo (and an rt that total_cmp orders as <= does)"""
    wide = np.flatnonzero(~((w["mass_hi"] - PRE_FILTER).astype(F32) <= w["mass_lo"]))
    if len(wide):
        i = int(wide[0])
        raise NotLayoutFree(f"{len(wide)} windows reach 0.1 or more below their mass_hi, the first [{w['mass_lo'][i]!r}, {w['mass_hi'][i]!r}]")
    if np.isnan(w["rt"]).any() or (np.signbit(w["rt"]) & (w["rt"] == 0)).any():
        raise NotLayoutFree("a window rt is NaN or -0.0")


def read_spectra(batches):
    """[(file, scan start time f32, masses f32 ascending, intensities, mobilities or None, order)] in the order the batches
    give the spectra; spectrum.rs:350-353 / :387-393: mass = (mz - PROTON) * 1.0, a stable sort on the total order, every
    column through the same permutation (`order`: the sorted peak's position as given)"""
    out = []
    for b in batches:
        for i in range(b.n):
            a, e = int(b.peak_off[i]), int(b.peak_off[i + 1])
            mass = ((np.asarray(b.mz[a:e], F32) - PROTON) * F32(1.0)).astype(F32)
            assert not np.isnan(mass).any() and not (np.signbit(mass) & (mass == 0)).any(), "total_cmp is <= without NaN and -0.0"
            order = np.argsort(mass, kind="stable")
            mob = None
            if b.mobility is not None and b.has_mobility[i]:
                mob = np.asarray(b.mobility[a:e], F32)[order]
            out.append((int(b.file_id[i]), F32(b.scan_start_time[i]), mass[order], np.asarray(b.intensities[a:e], F32)[order], mob, order))
    return out


def aligned_rt(scan_start_time, alignment):
    """lfq.rs:241; alignment = (file_id, max_rt, slope, intercept)"""
    return F32(F32(F32(scan_start_time) / F32(alignment[1])) * F32(alignment[2])) + F32(alignment[3])


def match(w, spectra, alignments):
    """every (spectrum, peak, window) that passes lfq.rs:668-673 (and :682-685 for a spectrum with a mobility column), ordered
    by (spectrum, sorted peak, window generation index): arrays spectrum, peak (position in ascending mass), raw_peak (position
    as given), window, and per match the spectrum's aligned rt and the peak's intensity"""
    require_layout_free(w)
    S, P, R, W, RT, IT = [], [], [], [], [], []
    for s, (fid, sst, mass, inten, mob, order) in enumerate(spectra):
        rt = aligned_rt(sst, alignments[fid])
        lo, hi = F32(rt - RT_TOL), F32(rt + RT_TOL)
        near = np.flatnonzero((w["rt"] <= hi) & (w["rt"] >= lo))
        if not len(near) or not len(mass):
            continue
        m = mass[:, None]
        ok = (m >= w["mass_lo"][near][None, :]) & (m <= w["mass_hi"][near][None, :])
        if mob is not None:  # spectrum.mobilities.is_empty() of :267 is false only with the column and at least one peak
            if "mobility_lo" not in w:
                raise ValueError("a spectrum has a mobility column, the windows have no mobility bounds")
            ok &= (w["mobility_hi"][near][None, :] >= mob[:, None]) & (w["mobility_lo"][near][None, :] <= mob[:, None])
        p, j = np.nonzero(ok)  # row-major: peak ascending, then window generation index ascending
        S.append(np.full(len(p), s, np.int64)), P.append(p), R.append(order[p]), W.append(near[j])
        RT.append(np.full(len(p), rt, F32)), IT.append(inten[p])
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)
    return dict(spectrum=cat(S, np.int64), peak=cat(P, np.int64), raw_peak=cat(R, np.int64), window=cat(W, np.int64),
                rt=cat(RT, F32), intensity=cat(IT, F32), file=np.array([sp[0] for sp in spectra], np.int64))


def match_pruned(w, spectra, alignments):
    """match() with a global prune: the same predicates on every pair, but only the pairs with
    f32(mass - 0.1f) <= mass_lo <= mass are formed, found by one np.searchsorted over all windows by mass_lo.  On a layout-free
    map the prune drops no match (step 3 of the proof above: mass <= mass_hi gives f32(mass - 0.1f) <= mass_lo, and the filter
    itself asks mass_lo <= mass).  Faster by two orders of magnitude; tests/test_lfq_trace_cpu.py holds it equal to match()."""
    require_layout_free(w)
    by_lo = np.argsort(w["mass_lo"], kind="stable")
    los = w["mass_lo"][by_lo]
    n = [len(sp[2]) for sp in spectra]
    cat = lambda xs, t: np.concatenate(xs).astype(t) if len(xs) else np.zeros(0, t)
    mass, inten = cat([sp[2] for sp in spectra], F32), cat([sp[3] for sp in spectra], F32)
    has = cat([np.full(k, sp[4] is not None) for k, sp in zip(n, spectra)], bool)
    mob = cat([sp[4] if sp[4] is not None else np.zeros(k, F32) for k, sp in zip(n, spectra)], F32)
    raw = cat([sp[5] for sp in spectra], np.int64)
    spec = np.repeat(np.arange(len(spectra)), n)
    peak = np.arange(len(mass)) - np.repeat(np.cumsum([0] + n[:-1]), n) if len(spectra) else np.zeros(0, np.int64)
    rt = np.array([aligned_rt(sp[1], alignments[sp[0]]) for sp in spectra], F32)
    a = np.searchsorted(los, (mass - PRE_FILTER).astype(F32), side="left")
    b = np.searchsorted(los, mass, side="right")
    k = np.maximum(b - a, 0)
    pair_peak = np.repeat(np.arange(len(mass)), k)                                  # index into the concatenated peaks
    win = by_lo[np.arange(int(k.sum())) - np.repeat(np.cumsum(k) - k, k) + np.repeat(a, k)]
    s = spec[pair_peak]
    m = mass[pair_peak]
    ok = (w["rt"][win] <= (rt + RT_TOL).astype(F32)[s]) & (w["rt"][win] >= (rt - RT_TOL).astype(F32)[s])
    ok &= (m >= w["mass_lo"][win]) & (m <= w["mass_hi"][win])
    if has.any():
        if "mobility_lo" not in w:
            raise ValueError("a spectrum has a mobility column, the windows have no mobility bounds")
        asked = has[pair_peak]
        ok &= ~asked | ((w["mobility_hi"][win] >= mob[pair_peak]) & (w["mobility_lo"][win] <= mob[pair_peak]))
    pair_peak, win = pair_peak[ok], win[ok]
    order = np.lexsort((win, pair_peak))       # (spectrum, sorted peak) is the concatenation's order; then generation index
    pair_peak, win = pair_peak[order], win[order]
    return dict(spectrum=spec[pair_peak].astype(np.int64), peak=peak[pair_peak].astype(np.int64), raw_peak=raw[pair_peak], window=win.astype(np.int64),
                rt=rt[spec[pair_peak]], intensity=inten[pair_peak], file=np.array([sp[0] for sp in spectra], np.int64))


def additions(w, m, n_files, combine):
    """Grid::add_entry (lfq.rs:538-550) of every match, as f32 arrays: the grid keys (sorted), and per addition — two per
    match, the lower bin first — its cell (grid * rows + row) * GRID_SIZE + bin and its f64 value, in the order of `m`"""
    win = m["window"]
    charge = np.zeros(len(win), np.int64) if combine else w["charge"][win]                 # :245-248
    keys, grid = np.unique(np.stack([w["peptide"][win], charge, w["decoy"][win].astype(np.int64)], axis=1), axis=0, return_inverse=True)
    grid = grid.reshape(-1)
    rows = n_files * N_ISOTOPES
    row = m["file"][m["spectrum"]] * N_ISOTOPES + w["isotope"][win]                        # :547
    rt_min = (w["rt"][win] - RT_TOL).astype(F32)                                           # :528, the entry's own rt
    step = (RT_TOL * F32(2.0)) / F32(GRID_SIZE)                                            # :525
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((m["rt"] - rt_min) / step)                                            # :539
    # `as usize` saturates: NaN and negatives to 0, anything large to the maximum, which .min(cols - 1) then caps
    bin_lo = np.where(q >= F32(GRID_SIZE - 1), GRID_SIZE - 1, np.where(q > 0, q, 0)).astype(np.int64)
    bin_lo = np.where(np.isnan(q), 0, bin_lo)
    bin_hi = np.minimum(bin_lo + 1, GRID_SIZE - 1)
    bin_lo_rt = (bin_lo.astype(F32) * step).astype(F32) + rt_min                           # :543
    interp = ((m["rt"] - bin_lo_rt) / step).astype(F32)                                    # :545
    with np.errstate(invalid="ignore", over="ignore"):
        v_lo = ((F32(1.0) - interp) * m["intensity"]).astype(F32).astype(np.float64)       # :548
        v_hi = (interp * m["intensity"]).astype(F32).astype(np.float64)                    # :549
    base = (grid * rows + row) * GRID_SIZE
    cell = np.stack([base + bin_lo, base + bin_hi], axis=1).reshape(-1)
    value = np.stack([v_lo, v_hi], axis=1).reshape(-1)
    # one peak, two windows of the same row: the order of those two additions would be the layout's
    rowkey = (m["spectrum"] * (int(m["peak"].max()) + 1 if len(win) else 1) + m["peak"]) * (len(keys) * rows) + grid * rows + row
    if len(np.unique(rowkey)) != len(rowkey):
        raise NotLayoutFree("a peak matches two windows of one (grid, file, isotope) row")
    return [tuple(int(x) for x in k[:2]) + (bool(k[2]),) for k in keys], cell, value


def fold(cell, value, n_cells, reverse=False):
    """every cell's additions folded left to right in f64 from 0.0, in the order given (or that order reversed): a stable
    sort by cell, then the k-th addition of every cell at once, k ascending.  Also the number of additions per cell."""
    if reverse:
        cell, value = cell[::-1], value[::-1]
    order = np.argsort(cell, kind="stable")
    c, v = cell[order], value[order]
    count = np.bincount(c, minlength=n_cells)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    rank = np.arange(len(c)) - start[c]
    by_rank = np.argsort(rank, kind="stable")
    per_rank = np.bincount(rank) if len(rank) else np.zeros(0, np.int64)
    acc = np.zeros(n_cells, np.float64)
    at = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for n in per_rank:                     # within one rank every cell occurs once: a plain gather-add-scatter
            sel = by_rank[at:at + n]
            acc[c[sel]] = acc[c[sel]] + v[sel]
            at += n
    return acc, count


def trace(w, spectra, alignments, n_files, combine, prune=False):
    """({(peptide, charge or 0, decoy): matrix[n_files * 3, 100] f64}, number of matches, the matches of match() — of
    match_pruned() with prune=True)"""
    m = (match_pruned if prune else match)(w, spectra, alignments)
    keys, cell, value = additions(w, m, n_files, combine)
    rows = n_files * N_ISOTOPES
    acc, _ = fold(cell, value, len(keys) * rows * GRID_SIZE)
    mats = acc.reshape(len(keys), rows, GRID_SIZE)
    return {k: mats[i] for i, k in enumerate(keys)}, len(m["window"]), m
