"""Seeded raw MS2 spectra that stress SpectrumProcessor::process (spectrum.rs:179-227, 279-412), for the preprocessing parity
tests (test_process_fuzz.py) — the host restatement and process_kernel against the oracle.

A spectrum is built from features until it has the requested number of peaks, then sorted by m/z (non-decreasing; equal m/z
values keep a random relative order, which the non-deisotoping heap makes visible in the output):
  - isolated peaks;
  - isotope envelopes at charges 1-8, satellites both below and above the parent intensity (only a lighter satellite is merged);
  - exact duplicates of an (m/z, intensity) pair;
  - equal m/z with different intensities;
and, per spectrum, optionally a few coarse intensity levels (ties in the intensity sort and in the heap) and zero intensities.
The peak counts sit on the kernel's edges: a wavefront (64), the bitonic sorts' power-of-two padding, the LDS / global-workspace
split at PROCESS_LDS_PEAKS = 2 048 raw peaks (process.hip), and a few spectra of 10 000 peaks or more."""
import numpy as np

NEUTRON = np.float32(1.00335)
# raw peak counts at the edges of process_kernel
EDGE_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4096, 4097)
HUGE_COUNTS = (10000, 12289, 16385)
LDS_PEAKS = 2048  # process.hip: PROCESS_LDS_PEAKS


def peak_count(rng, huge=0.03):
    """A raw peak count: an edge count, a count near one, or (rarely) a huge one."""
    u = rng.random()
    if u < huge:
        return int(rng.choice(HUGE_COUNTS))
    if u < 0.7:
        return int(rng.choice(EDGE_COUNTS))
    return int(rng.integers(3, 3000))


def raw_peaks(rng, n, mz_lo=100.0, mz_hi=2000.0, coarse=None, zeros=None):
    """(mz[n] f32 non-decreasing, intensity[n] f32).  coarse / zeros: None = drawn."""
    if n == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    mz, it = [], []
    have = 0
    while have < n:
        u = rng.random()
        base = np.float32(rng.uniform(mz_lo, mz_hi))
        parent = np.float32(rng.lognormal(8.0, 1.5))
        if u < 0.45:  # isolated peak
            m, i = [base], [parent]
        elif u < 0.8:  # an isotope envelope: 1-4 satellites at +k * NEUTRON / z, a few ppm off
            z = int(rng.integers(1, 9))
            k = np.arange(1, int(rng.integers(2, 6)), dtype=np.float32)
            jitter = np.float32(1.0) + rng.normal(0.0, 2e-6, len(k)).astype(np.float32)
            m = [base] + list((base + k * (NEUTRON / np.float32(z))) * jitter)
            # a satellite is usually lighter than the one before it, sometimes heavier (not merged into the envelope)
            f = np.where(rng.random(len(k)) < 0.8, rng.uniform(0.2, 0.95, len(k)), rng.uniform(1.05, 2.0, len(k)))
            i = [parent] + list(parent * np.cumprod(f).astype(np.float32))
        elif u < 0.9:  # exact duplicates of (m/z, intensity)
            c = int(rng.integers(2, 4))
            m, i = [base] * c, [parent] * c
        else:  # equal m/z, different intensities
            c = int(rng.integers(2, 5))
            m, i = [base] * c, list(parent * rng.uniform(0.1, 3.0, c).astype(np.float32))
        mz += m
        it += i
        have += len(m)
    mz = np.asarray(mz, np.float32)
    it = np.asarray(it, np.float32)
    if len(mz) > n:  # drop random peaks (some envelopes lose a member)
        pick = np.sort(rng.choice(len(mz), n, replace=False))
        mz, it = mz[pick], it[pick]
    if coarse is None:
        coarse = rng.random() < 0.35
    if coarse:  # a few intensity levels: ties everywhere in the intensity order
        levels = int(rng.integers(2, 9))
        top = np.float32(it.max())
        it = (np.ceil(it / top * np.float32(levels)) * np.float32(top / np.float32(levels))).astype(np.float32)
    if zeros is None:
        zeros = rng.random() < 0.2
    if zeros:
        it[rng.random(n) < 0.1] = np.float32(0.0)
    shuffle = rng.permutation(n)  # equal m/z values in a random relative order
    mz, it = mz[shuffle], it[shuffle]
    o = np.argsort(mz, kind="stable")
    return np.ascontiguousarray(mz[o]), np.ascontiguousarray(it[o])


def precursor_charge(rng):
    """0 (unknown: max charge 3, spectrum.rs:289-293) or 1-8."""
    return 0 if rng.random() < 0.3 else int(rng.integers(1, 9))


def take_top_n(rng, n):
    """One of {1, 2, 63, 64, 65, n-1, n, n+1, 150, 65 535} (never 0: take_top_n is at least 1 here)."""
    c = [1, 2, 63, 64, 65, max(n - 1, 1), max(n, 1), n + 1, 150, 65535]
    return int(c[int(rng.integers(0, len(c)))])


def min_deisotope_mz(rng, mz_sets):
    """0, a value inside the spectra, exactly an existing peak's m/z, or a value above every peak."""
    u = rng.random()
    peaks = [m for m in mz_sets if len(m)]
    if u < 0.3 or not peaks:
        return 0.0
    if u < 0.55:
        m = peaks[int(rng.integers(0, len(peaks)))]
        return float(m[int(rng.integers(0, len(m)))])  # (an f32 value: exactly representable)
    if u < 0.85:
        return float(np.float32(rng.uniform(150.0, 1900.0)))
    return float(np.float32(max(float(m[-1]) for m in peaks) + 1.0))
