"""Named worlds of the precursor-purity tests: MS1 batches and queries built to sit on the seams of the kernel — sizes
round the wavefront and the LDS chunk, window populations round 64, peaks on and next to every bound, orders and values that a
reordered or partial sum would get wrong.  Shared by tests/test_purity_cpu.py (host emulation) and tests/test_gpu_purity.py
(device); the expected values come from tests/purity_reference.py, computed once per world."""
import functools
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

import purity_reference as REF
from sage_amd.api import RawBatch

F = np.float32
NAN = float("nan")
FIELDS = ("n_window", "n_matched", "total", "matched", "below", "purity")


@dataclass
class World:
    batches: List[RawBatch]
    ms1_index: np.ndarray
    mz: np.ndarray
    charge: np.ndarray
    lo: Optional[np.ndarray] = None
    hi: Optional[np.ndarray] = None
    ppm: float = 10.0
    max_isotope: int = 4
    default: tuple = (-0.5, 0.5)
    sorted_spectra: Optional[int] = None    # spectra with a query that are non-decreasing and NaN-free / the others, where a test
    scanned_spectra: Optional[int] = None   # asserts the routes
    notes: dict = field(default_factory=dict)


def batch(spectra, file_id=0, times=None) -> RawBatch:
    """spectra: [(mz, intensity)] as given (no sorting here)"""
    n = len(spectra)
    off = np.zeros(n + 1, np.uint64)
    for i, (m, _) in enumerate(spectra):
        off[i + 1] = off[i] + len(m)
    cat = lambda k: np.concatenate([np.asarray(s[k], F) for s in spectra]) if n else np.zeros(0, F)
    nan = np.full(n, np.nan, F)
    return RawBatch.from_arrays([f"scan={i + 1}" for i in range(n)], off, cat(0), cat(1), np.zeros(n, F), np.zeros(n, np.uint8), nan, nan,
                                np.arange(n, dtype=F) if times is None else times, nan, np.full(n, file_id, np.uint32))


def ulps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def bounds_of(mz, z, lo, hi, ppm, max_isotope, default=(-0.5, 0.5)):
    """every bound of a query as the contract computes it: (wlo, whi), the envelope's, the `below` interval's"""
    mz, t = F(mz), F(ppm)
    if np.isnan(lo) or np.isnan(hi):
        lo, hi = default
    out = [F(mz + F(lo)), F(mz + F(hi))]
    if z == 0:
        out += list(REF.ppm_bounds(mz, t))
    else:
        for k in range(max_isotope + 1):
            out += list(REF.ppm_bounds(mz + (F(k) * REF.NEUTRON) / F(z), t))
        out += list(REF.ppm_bounds(mz - REF.NEUTRON / F(z), t))
    return out


def _queries(rng, counts, spectra_mz, planted, nan_every=3):
    """counts[s] queries on spectrum s: in turn a planted precursor with its charge (else a peak of the spectrum) and an m/z anywhere
    in the range, with charges 0..6 in turn; every nan_every-th pair of offsets NaN (the default pair), the others drawn"""
    idx, mz, z, lo, hi = [], [], [], [], []
    for s, c in enumerate(counts):
        m = spectra_mz[s]
        for j in range(c):
            idx.append(s)
            finite = m[np.isfinite(m)] if len(m) else m
            z.append(len(idx) % 7)
            if planted[s] and j % 2 == 0:
                mz.append(planted[s][j // 2 % len(planted[s])][0])
                z[-1] = planted[s][j // 2 % len(planted[s])][1]
            elif len(finite) and j % 2 == 0:
                mz.append(F(finite[rng.integers(len(finite))]))
            else:
                mz.append(F(rng.uniform(400.0, 430.0)))
            if len(idx) % nan_every == 0:
                lo.append(NAN)
                hi.append(NAN if len(idx) % 2 else 0.7)  # (one NaN is enough for the default pair)
            else:
                lo.append(-rng.uniform(0.1, 1.0))
                hi.append(rng.uniform(0.1, 1.0))
    return (np.array(idx, np.uint64), np.array(mz, F), np.array(z, np.uint8), np.array(lo, F), np.array(hi, F))


def _with_envelopes(rng, base_mz, n_plant):
    """base peaks + planted isotope envelopes (f32 centres, some a few ppm off) of random precursors among them, and those
    precursors' (m/z, charge)"""
    if not len(base_mz) or not n_plant:
        return base_mz, []
    extra, planted = [], []
    for _ in range(n_plant):
        m, z = F(base_mz[rng.integers(len(base_mz))]), int(rng.integers(1, 7))
        planted.append((m, z))
        for k in range(-1, 6):
            c = m + (F(abs(k)) * REF.NEUTRON) / F(z) * F(1 if k >= 0 else -1)
            extra.append(c * F(1.0 + rng.normal(0.0, 6.0) * 1e-6))
    return np.concatenate([base_mz, np.array(extra, F)]), planted


def sizes(seed=1, k=4, shuffle_peaks=False):
    """spectrum sizes round the wavefront (64), the LDS chunk (2048) and beyond a compute unit's LDS (30 000 peaks), queries per
    spectrum 0 / 1 / 63 / 64 / 65 / 300, three batches with queries crossing their seams, queries shuffled, some without MS1"""
    rng = np.random.default_rng(seed)
    want = [0, 1, 63, 64, 65, 2047, 2048, 2049, 5000, 30000]
    counts = [1, 63, 64, 65, 300, 1, 2, 0, 5, 8]
    spectra, planted = [], []
    for n in want:
        plant = min(n // 40, 40)
        base = rng.uniform(400.0, 430.0, max(n - 7 * plant, 0)).astype(F)
        m, precursors = _with_envelopes(rng, base, plant)
        planted.append(precursors)
        assert len(m) == n
        m = rng.permutation(m) if shuffle_peaks else np.sort(m)
        spectra.append((m.astype(F), rng.lognormal(8.0, 1.5, n).astype(F)))
    idx, mz, z, lo, hi = _queries(rng, counts, [s[0] for s in spectra], planted)
    none = 5
    idx = np.concatenate([idx, np.full(none, REF.NO_MS1, np.uint64)])
    mz = np.concatenate([mz, np.full(none, 415.0, F)])
    z = np.concatenate([z, np.full(none, 2, np.uint8)])
    lo, hi = np.concatenate([lo, np.full(none, -0.4, F)]), np.concatenate([hi, np.full(none, 0.4, F)])
    p = rng.permutation(len(idx))
    batches = [batch(spectra[:3]), batch(spectra[3:4]), batch([]), batch(spectra[4:])]
    with_query = sum(1 for c in counts if c)
    return World(batches, idx[p], mz[p], z[p], lo[p], hi[p], max_isotope=k,
                 sorted_spectra=2 if shuffle_peaks else with_query,  # (no peak, or one: in order however they were shuffled)
                 scanned_spectra=with_query - 2 if shuffle_peaks else 0)


def populations(k=4, shuffled=False):
    """windows of +-0.5 Da holding 0, 1, 2, 63, 64, 65, 129 and 1 000 peaks, the precursor's own peak among them"""
    rng = np.random.default_rng(7)
    pops = [0, 1, 2, 63, 64, 65, 129, 1000]
    mzs, centres = [rng.uniform(100.0, 300.0, 500)], []
    for j, c in enumerate(pops):
        centre = F(500.0 + 10.0 * j)
        centres.append(centre)
        if c:
            mzs.append(np.concatenate([[centre], centre + rng.uniform(-0.3, 0.3, c - 1)]))
    m = np.concatenate(mzs).astype(F)
    m = rng.permutation(m) if shuffled else np.sort(m)
    it = rng.lognormal(8.0, 1.0, len(m)).astype(F)
    n = len(pops)
    w = World([batch([(m, it)])], np.zeros(n, np.uint64), np.array(centres, F), np.full(n, 2, np.uint8), max_isotope=k,
              sorted_spectra=0 if shuffled else 1, scanned_spectra=1 if shuffled else 0, notes={"populations": pops})
    return w


def edges(k=4, ppm=10.0, shuffled=False):
    """peaks exactly on wlo, whi, every elo_k / ehi_k and the `below` bounds, and 1-3 ulps either side; charges 0..6"""
    rng = np.random.default_rng(11)
    qs = [(F(500.25 + 37.5 * z), z, (-0.7, 0.9) if z % 2 else (NAN, NAN)) for z in range(7)]
    peaks = []
    for mz, z, (lo, hi) in qs:
        for b in bounds_of(mz, z, lo, hi, ppm, k):
            peaks += [ulps(b, d) for d in range(-3, 4)]
    m = np.array(peaks, F)
    m = rng.permutation(m) if shuffled else np.sort(m)
    it = rng.lognormal(8.0, 1.0, len(m)).astype(F)
    n = len(qs)
    return World([batch([(m, it)])], np.zeros(n, np.uint64), np.array([q[0] for q in qs], F), np.array([q[1] for q in qs], np.uint8),
                 np.array([q[2][0] for q in qs], F), np.array([q[2][1] for q in qs], F), ppm=ppm, max_isotope=k,
                 sorted_spectra=0 if shuffled else 1, scanned_spectra=1 if shuffled else 0)


def two_k():
    """a tolerance so wide (400 ppm at charge 6) that neighbouring centres' bounds overlap: a peak meeting two k counts once"""
    w = edges(k=4, ppm=400.0)
    w.notes["overlap"] = True
    return w


def equal_mz():
    """runs of equal m/z (non-decreasing: the sorted route), among them the precursor's"""
    rng = np.random.default_rng(13)
    m = np.sort(np.repeat(rng.uniform(600.0, 604.0, 40).astype(F), rng.integers(1, 9, 40)))
    it = rng.lognormal(8.0, 1.0, len(m)).astype(F)
    q = np.unique(m)[::3]
    n = len(q)
    return World([batch([(m, it)])], np.zeros(n, np.uint64), q.astype(F), (np.arange(n) % 5).astype(np.uint8), sorted_spectra=1,
                 scanned_spectra=0)


def nan_mz():
    """three sorted spectra, the middle one with a NaN m/z inside a window: that spectrum alone is scanned"""
    rng = np.random.default_rng(17)
    spectra = []
    for s in range(3):
        m = np.sort(rng.uniform(700.0, 703.0, 200).astype(F))
        if s == 1:
            m[100] = np.nan
        spectra.append((m, rng.lognormal(8.0, 1.0, 200).astype(F)))
    idx = np.repeat(np.arange(3, dtype=np.uint64), 4)
    mz = np.array([spectra[int(s)][0][90 + 7 * j] for j, s in enumerate(idx)], F)
    return World([batch(spectra[:2]), batch(spectra[2:])], idx, mz, np.full(len(idx), 2, np.uint8), sorted_spectra=2, scanned_spectra=1)


def odd_intensities(shuffled=False):
    """NaN, +-inf, negative and -0.0 intensities inside the windows: they pass through the sums as written"""
    rng = np.random.default_rng(19)
    specials = [np.nan, np.inf, -np.inf, -5.0, -0.0, 0.0]
    spectra, mzq = [], []
    for s, special in enumerate(specials + [None, None]):
        m = np.sort(rng.uniform(800.0, 800.8, 30).astype(F))
        it = rng.lognormal(8.0, 1.0, 30).astype(F)
        if special is not None:
            it[[3, 15]] = special
        elif s == len(specials):
            it[:] = -0.0           # every sum stays +0.0 + -0.0 = +0.0; purity 0 / 0
        else:
            it[10], it[20] = np.inf, -np.inf  # total NaN
        if shuffled:
            p = rng.permutation(30)
            m, it = m[p], it[p]
        spectra.append((m, it.astype(F)))
        mzq.append(F(800.4))
    n = len(spectra)
    return World([batch(spectra)], np.arange(n, dtype=np.uint64), np.array(mzq, F), np.full(n, 1, np.uint8), sorted_spectra=0 if shuffled else n,
                 scanned_spectra=n if shuffled else 0)


def order_case():
    """windows holding [2^53, 1, 1] and [1, 1, 2^53]: in position order the totals are 2^53 and 2^53 + 2 (f64, round to even)"""
    big = F(2.0 ** 53)
    m = np.array([900.0, 900.1, 900.2], F)
    spectra = [(m, np.array([big, 1.0, 1.0], F)), (m, np.array([1.0, 1.0, big], F)),
               (m[::-1].copy(), np.array([big, 1.0, 1.0], F)), (m[::-1].copy(), np.array([1.0, 1.0, big], F))]
    return World([batch(spectra)], np.arange(4, dtype=np.uint64), np.full(4, 900.1, F), np.full(4, 0, np.uint8), sorted_spectra=2,
                 scanned_spectra=2, notes={"totals": [2.0 ** 53, 2.0 ** 53 + 2.0, 2.0 ** 53, 2.0 ** 53 + 2.0]})


def no_ms1_only():
    n = 3
    return World([], np.full(n, REF.NO_MS1, np.uint64), np.full(n, 500.0, F), np.full(n, 2, np.uint8), sorted_spectra=0, scanned_spectra=0)


def no_queries():
    w = nan_mz()
    return World(w.batches, np.zeros(0, np.uint64), np.zeros(0, F), np.zeros(0, np.uint8), sorted_spectra=0, scanned_spectra=0)


WORLDS = {
    "sizes_k4": lambda: sizes(k=4),
    "sizes_k0": lambda: sizes(seed=2, k=0),
    "sizes_k16": lambda: sizes(seed=3, k=16),
    "sizes_unsorted": lambda: sizes(seed=4, k=4, shuffle_peaks=True),
    "populations_k4": lambda: populations(4),
    "populations_k16": lambda: populations(16),
    "populations_unsorted": lambda: populations(4, shuffled=True),
    "edges_k4": lambda: edges(4),
    "edges_k0": lambda: edges(0),
    "edges_k16": lambda: edges(16),
    "edges_unsorted": lambda: edges(4, shuffled=True),
    "two_k": two_k,
    "equal_mz": equal_mz,
    "nan_mz": nan_mz,
    "odd_intensities": odd_intensities,
    "odd_intensities_unsorted": lambda: odd_intensities(shuffled=True),
    "order_case": order_case,
    "no_ms1_only": no_ms1_only,
    "no_queries": no_queries,
}
NAMES = list(WORLDS)


@functools.lru_cache(maxsize=None)
def world(name) -> World:
    return WORLDS[name]()


@functools.lru_cache(maxsize=None)
def reference(name) -> dict:
    w = world(name)
    want = REF.run(w.batches, w.ms1_index, w.mz, w.charge, w.lo, w.hi, w.ppm, w.max_isotope, w.default)
    for v in want.values():
        v.setflags(write=False)
    return want


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_equal(got: dict, want: dict, name):
    """every output bit (a NaN must be the NaN the contract's operations produce)"""
    for k in FIELDS:
        g, w = np.asarray(got[k]), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.flatnonzero(bits(g) != bits(w))
        # (the sign and payload of a NaN that arithmetic produced are not the contract's: inf - inf is a NaN on every machine)
        bad = [i for i in bad if not (np.isnan(g[i]) and np.isnan(w[i]))]
        assert not bad, (name, k, bad[:5], g[bad[:5]], w[bad[:5]])
