"""A plain sequential restatement of the precursor-purity contract (sage_amd/csrc/purity.h) and of assign_ms1.
numpy f32 scalars for every m/z operation (one rounding each), Python floats (IEEE f64) for the sums, one peak after another in
the order given.  It knows nothing of routes, sorting or grouping."""
import numpy as np

F = np.float32
NEUTRON = F(1.00335)
NO_MS1 = 0xFFFFFFFFFFFFFFFF


def ppm_bounds(center, t):
    """Tolerance::bounds of Ppm(-t, t) (mass.rs:21-35): (center * lo) / 1e6, then center + delta, in f32."""
    with np.errstate(all="ignore"):
        dlo = center * F(-t) / F(1000000.0)
        dhi = center * F(t) / F(1000000.0)
        return center + dlo, center + dhi


def query(mz_of, intensity_of, mz, z, lo, hi, ppm=10.0, max_isotope=4, default=(-0.5, 0.5)):
    """One query over one spectrum (None: no MS1) -> (n_window, n_matched, total, matched, below, purity as np.float32)."""
    if mz_of is None:
        return 0, 0, 0.0, 0.0, 0.0, F(-1.0)
    mz, lo, hi, t = F(mz), F(lo), F(hi), F(ppm)
    z = int(z)
    with np.errstate(all="ignore"):
        if np.isnan(lo) or np.isnan(hi):
            lo, hi = F(default[0]), F(default[1])
        wlo, whi = mz + lo, mz + hi
        centres = [mz] if z == 0 else [mz + (F(k) * NEUTRON) / F(z) for k in range(max_isotope + 1)]
        envelope = [ppm_bounds(c, t) for c in centres]
        below_bounds = None if z == 0 else ppm_bounds(mz - NEUTRON / F(z), t)
    # the tests peak by peak (elementwise f32 comparisons; a NaN compares false), then each sum over its peaks one after another
    p = np.asarray(mz_of, F)
    v = np.asarray(intensity_of, F)
    with np.errstate(all="ignore"):
        in_window = (wlo <= p) & (p <= whi)
        on_envelope = np.zeros(len(p), bool)
        for a, b in envelope:
            on_envelope |= (a <= p) & (p <= b)
        in_below = np.zeros(len(p), bool) if below_bounds is None else (below_bounds[0] <= p) & (p <= below_bounds[1])
    n_window, n_matched = int(in_window.sum()), int((in_window & on_envelope).sum())
    total = matched = below = 0.0
    for i in np.flatnonzero(in_window):
        total += float(v[i])
    for i in np.flatnonzero(in_window & on_envelope):
        matched += float(v[i])
    for i in np.flatnonzero(in_below):
        below += float(v[i])
    if n_window == 0:
        return 0, 0, 0.0, 0.0, 0.0, F(-1.0)  # (`below` too: without a peak in the window every sum is +0.0)
    with np.errstate(all="ignore"):
        purity = F(np.float64(matched) / np.float64(total))
    return n_window, n_matched, total, matched, below, purity


def spectra_of(batches):
    """[(mz, intensity)] of every spectrum, counted through the batches in order."""
    out = []
    for b in batches:
        for i in range(b.n):
            a, e = int(b.peak_off[i]), int(b.peak_off[i + 1])
            out.append((b.mz[a:e], b.intensities[a:e]))
    return out


def run(batches, ms1_index, precursor_mz, charge, isolation_lo=None, isolation_hi=None, ppm=10.0, max_isotope=4, default=(-0.5, 0.5)):
    """Every query -> dict of arrays named like api.PurityResult's fields."""
    spectra = spectra_of(batches)
    n = len(ms1_index)
    nan = float("nan")
    rows = []
    for i in range(n):
        s = int(ms1_index[i])
        m, it = (None, None) if s == NO_MS1 else spectra[s]
        rows.append(query(m, it, precursor_mz[i], charge[i], nan if isolation_lo is None or isolation_hi is None else isolation_lo[i],
                          nan if isolation_lo is None or isolation_hi is None else isolation_hi[i], ppm, max_isotope, default))
    col = lambda k, dt: np.array([r[k] for r in rows], dtype=dt)
    return {"n_window": col(0, np.uint32), "n_matched": col(1, np.uint32), "total": col(2, np.float64), "matched": col(3, np.float64),
            "below": col(4, np.float64), "purity": col(5, np.float32)}


def assign_ms1(batches, file_id, scan_start_time):
    """Of the spectra of the same file, the greatest scan_start_time <= t; among equal times the later in the given order."""
    spectra = []
    for b in batches:
        for i in range(b.n):
            spectra.append((int(b.file_id[i]), F(b.scan_start_time[i])))
    out = []
    for f, t in zip(file_id, scan_start_time):
        best, best_t = NO_MS1, None
        for s, (sf, st) in enumerate(spectra):
            if sf == int(f) and bool(st <= F(t)) and (best_t is None or bool(st >= best_t)):
                best, best_t = s, st
        out.append(best)
    return np.array(out, dtype=np.uint64)
