"""Sequential restatement of sage's TMT quantification, in numpy f32, for the device tests (tests/test_gpu_tmt.py).

  * select_most_intense_peak with an offset (spectrum.rs:134-159): Tolerance::bounds (mass.rs:21-35) in f32, the offset added
    to each bound, binary_search_slice's range (database.rs:549-561, total_cmp, the minus-one rule), then the scan that keeps
    the LAST peak with intensity >= the running maximum, starting from 0.0;
  * find_reporter_ions (tmt.rs:193-214): that search per label with offset -PROTON, intensity or None;
  * the processing of spectra at levels other than 2 (spectrum.rs:380-412): mass = (mz - PROTON) * 1.0, stable sort by
    total_cmp;
  * quantify's row rules (tmt.rs:314-352): level 1 no row, level 2 the spectrum id, other levels precursors.first().spectrum_ref;
  * the reader's signal-to-noise division (mzml.rs:371-381): intensity[i] /= noise[i] over the shorter length, f32.
Nothing here is shared with the product code.
"""
import numpy as np

F32 = np.float32
PROTON = F32(1.0072764)


def bounds(center, tol):
    """Tolerance::bounds: (kind, lo, hi) with kind "ppm" | "pct" | "da"."""
    kind, lo, hi = tol
    c, lo, hi = F32(center), F32(lo), F32(hi)
    with np.errstate(all="ignore"):
        if kind == "ppm":
            return F32(c + F32(F32(c * lo) / F32(1e6))), F32(c + F32(F32(c * hi) / F32(1e6)))
        if kind == "pct":
            return F32(c + F32(F32(c * lo) / F32(100.0))), F32(c + F32(F32(c * hi) / F32(100.0)))
        return F32(c + lo), F32(c + hi)


def total_key(x):
    """f32::total_cmp as int64 keys"""
    b = np.asarray(x, dtype=F32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def select_most_intense_peak(masses, intensities, center, tol, offset=None):
    masses = np.asarray(masses, dtype=F32)
    intensities = np.asarray(intensities, dtype=F32)
    lo, hi = bounds(center, tol)
    off = F32(0.0) if offset is None else F32(offset)
    with np.errstate(all="ignore"):
        lo, hi = F32(lo + off), F32(hi + off)
    keys = total_key(masses)
    left = max(int(np.searchsorted(keys, total_key(lo), side="left")) - 1, 0)        # partition_point(< lo), saturating - 1
    right = left + int(np.searchsorted(keys[left:], total_key(hi), side="right"))     # partition_point(<= hi) over [left..]
    best, max_int = None, F32(0.0)
    for idx in range(left, right):
        m = masses[idx]
        if m >= lo and m <= hi and intensities[idx] >= max_int:
            max_int = intensities[idx]
            best = idx
    return best


def find_reporter_ions(masses, intensities, labels, tol=("ppm", -20.0, 20.0)):
    """[(intensity or None, index or None)] per label"""
    out = []
    for lab in np.asarray(labels, dtype=F32):
        i = select_most_intense_peak(masses, intensities, lab, tol, -PROTON)
        out.append((None, None) if i is None else (F32(intensities[i]), i))
    return out


def process_other_level(mz, intensity):
    """spectrum.rs:380-412 for ms_level != 2 (no mobility): (masses, intensities, raw position of every sorted peak)"""
    mz = np.asarray(mz, dtype=F32)
    it = np.asarray(intensity, dtype=F32)
    with np.errstate(all="ignore"):
        mass = ((mz - PROTON) * F32(1.0)).astype(F32)
    order = np.argsort(total_key(mass), kind="stable")
    return mass[order], it[order], order


def quantify_spectrum(level, masses, intensities, labels, tol=("ppm", -20.0, 20.0), raw_position=None):
    """One TmtQuant's peaks (tmt.rs:336-344): (intensity[L] f32 with 0.0 for None, index[L] i32 with -1 for None).  The index
    is the position in `masses` or, given raw_position (the sort's permutation), the raw position."""
    res = find_reporter_ions(masses, intensities, labels, tol)
    val = np.array([F32(0.0) if v is None else v for v, _ in res], dtype=F32)
    idx = np.array([-1 if i is None else (int(raw_position[i]) if raw_position is not None else i) for _, i in res], dtype=np.int32)
    return val, idx


def row_spec_id(level, spectrum_id, precursor_ref):
    """tmt.rs:330-335: None (no row) at level 1"""
    if level == 1:
        return None
    return spectrum_id if level == 2 else (precursor_ref or "")


def signal_to_noise(intensity, noise):
    it = np.array(intensity, dtype=F32)
    if noise is None or len(noise) == 0:
        return it
    k = min(len(it), len(noise))
    with np.errstate(all="ignore"):
        it[:k] = it[:k] / np.asarray(noise, dtype=F32)[:k]
    return it


def min_deisotope_mz(labels):
    """runner.rs:398-403: labels.last() * (1.0 + 20E-6) in f32, 0.0 without labels"""
    labels = np.asarray(labels, dtype=F32)
    return F32(labels[-1] * F32(F32(1.0) + F32(20e-6))) if len(labels) else F32(0.0)


def self_test():
    # spectrum.rs:589-605: the offset shifts the window onto the proton-subtracted mass
    label = F32(126.127726)
    masses = np.array([label - PROTON - F32(0.01), label - PROTON, label - PROTON + F32(0.01)], dtype=F32)
    assert select_most_intense_peak(masses, [10.0, 100.0, 50.0], label, ("da", -0.005, 0.005), -PROTON) == 1
    # ties go to the later peak; NaN never; -0.0 counts; nothing in the window: None
    m = np.array([100.0, 100.0, 100.0], dtype=F32)
    assert select_most_intense_peak(m, [5.0, 5.0, np.nan], 100.0, ("da", -1, 1)) == 1
    assert select_most_intense_peak(m, [-0.0, np.nan, -1.0], 100.0, ("da", -1, 1)) == 0
    assert select_most_intense_peak(m, [-1.0, -2.0, np.nan], 100.0, ("da", -1, 1)) is None
    assert select_most_intense_peak(m, [1.0, 1.0, 1.0], 300.0, ("da", -1, 1)) is None
    return True
