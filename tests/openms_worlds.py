"""Worlds AIMED at OpenMSHyperScore's f32 `ln_1p(summed_b + summed_y)` (scoring.rs:187-199) — TEST INFRASTRUCTURE, CPU only.

An already processed SpectrumBatch hands its intensities to the scorer as they are.  A spectrum whose only matching peak is ONE
fragment of its peptide, scored with min_matched_peaks = 1, has summed_b + summed_y equal to that peak's f32 intensity, so the
argument of ln_1p can be set to any bit pattern that select_most_intense_peak accepts (spectrum.rs:134-159: `intensity >= 0`:
+-0, every positive number, +inf).  NaN and every negative intensity are never matched: a summed intensity that is NaN, -1, below
-1 or in (-1, 0) cannot be produced through the kernels — those arguments are held on the shared function itself, exhaustively
(tests/test_ln1pf_cpu.py), and here the worlds only show that such peaks give no PSM.

The database is hand-built (tests/index_cases.py): a few hundred peptides that all start with alanine, ion kinds b and y,
min_ion_index 0, so that b1 is the same m/z for every peptide (a peak there matches ALL of them: hundreds of tied candidates,
which the k-select has to trim — the tie route into the retry pass).  A `home` peptide has a b ion and a y ion that lie 0.05 Da
away from every other ion of the whole database: a peak there is one fragment of one peptide under any precursor window.

Expected hyperscores come from the CPU alone: (double)ref_ln1pf(si) + lnfact(matched_b) + lnfact(matched_y), ref_ln1pf being
libquadmath's log1pq rounded once (tests/hostemu/ln1pf_emu.cpp), lnfact Stirling's series over the oracle's correctly rounded
ln (oracle_lib.ln_batch(x, 1)), both sums in f64 from the left as scoring.rs writes them."""
import math

import numpy as np

import oracle_lib
import test_ln1pf_cpu as LN
from index_cases import AA, BY, Pep, database
from index_reference import F32, IndexReference
from index_search_worlds import BucketedDb, holding_precursor, tol_tuple
from sage_amd.api import ScorerParams, SpectrumBatch, Tolerance

N_PEPTIDES = 320
ISOLATION = 0.05          # Da between a home's ion and every other ion of the database
MONO_GAP = 0.2            # Da between a home's mass and every other peptide's
FRAGMENT_TOL = Tolerance("ppm", -10.0, 10.0)
NARROW = Tolerance("ppm", -10.0, 10.0)
MAX_SPECTRA = 4096
FLT_MAX = 0x7F7FFFFF
INF = 0x7F800000


def f32_of(bits):
    return np.asarray(bits, dtype=np.uint32).view(F32)


def bits_of(x):
    return np.asarray(x, dtype=F32).view(np.uint32)


# ---- expected values -----------------------------------------------------------------------------------------------------------
def lnfact(n):
    """scoring.rs:170-177 over the oracle's correctly rounded ln"""
    if n == 0:
        return 1.0
    x = float(n)
    ln_x, ln_2pix = (float(v) for v in oracle_lib.ln_batch(np.array([x, math.pi * 2.0 * x]), 1))
    return x * ln_x - x + 0.5 * ln_x + 0.5 * ln_2pix


_LNFACT = {}


def expected_hyperscore(si_bits, matched_b, matched_y):
    """ScoreType::OpenMSHyperScore for an array of summed intensities (bit patterns) -> f64 array"""
    for n in (matched_b, matched_y):
        if n not in _LNFACT:
            _LNFACT[n] = lnfact(n)
    with np.errstate(all="ignore"):
        s = LN.ref_ln1pf(si_bits).view(F32).astype(np.float64) + _LNFACT[matched_b] + _LNFACT[matched_y]
    return np.where(np.isfinite(s), s, 255.0)


# ---- the database --------------------------------------------------------------------------------------------------------------
class OpenMsWorld:
    pass


_world = None


def world():
    global _world
    if _world is None:
        _world = _build()
    return _world


def _build():
    rng = np.random.default_rng(2031)
    letters = np.frombuffer(AA, np.uint8)
    peps = [Pep(b"A" + letters[rng.integers(0, len(letters), int(k))].tobytes()) for k in rng.integers(6, 12, N_PEPTIDES)]
    w = OpenMsWorld()
    w.db = db = database(peps, BY, 0)
    w.ref = ref = IndexReference(db)
    w.bucketed = BucketedDb(db, ref, 64)
    w.oracle = w.bucketed.oracle()
    mono = db.pep_mono.astype(np.float64)
    ions = np.sort(ref.ions.astype(np.float64))
    w.b1 = F32(ref.ions[0])
    assert all(ref.ions[int(ref.ion_off[p])] == w.b1 for p in range(db.n_peptides)), "b1 is the same m/z for every peptide"
    w.homes = []   # (peptide, its isolated b ion, its isolated y ion)
    for p in range(db.n_peptides):
        gaps = np.abs(np.delete(mono, p) - mono[p])
        if gaps.min() < MONO_GAP:
            continue
        m = (int(ref.ion_off[p + 1]) - int(ref.ion_off[p])) // 2
        own = []
        for k in range(2):
            found = None
            for j in range(1 if k == 0 else 0, m):   # (not b1)
                e = float(ref.ions[int(ref.ion_off[p]) + k * m + j])
                a, z = np.searchsorted(ions, e - ISOLATION), np.searchsorted(ions, e + ISOLATION)
                if z - a == 1 and e > 100.0:
                    found = F32(e)
                    break
            own.append(found)
        if own[0] is not None and own[1] is not None:
            w.homes.append((p, own[0], own[1]))
    assert len(w.homes) >= 60, len(w.homes)
    span = float(mono[-1] - mono[0]) + 50.0
    w.whole = Tolerance("da", -span, span)
    w.middle_mz = holding_precursor(tol_tuple(w.whole), 2, F32(0.5 * (mono[0] + mono[-1])))
    return w


def make_batch(w, plans):
    """plans: [(precursor m/z, [(peak mass, intensity bits)])] -> SpectrumBatch (charge 2: fragment charge 1 only, scoring.rs:239-247)"""
    off, masses, intens, tic = [0], [], [], []
    for _, peaks in plans:
        peaks = sorted(peaks, key=lambda pk: float(pk[0]))
        masses += [pk[0] for pk in peaks]
        it = f32_of([pk[1] for pk in peaks])
        intens.append(it)
        off.append(off[-1] + len(peaks))
        with np.errstate(all="ignore"):
            tic.append(np.cumsum(it, dtype=F32)[-1] if len(it) else F32(0.0))
    k = len(plans)
    return SpectrumBatch(np.array(off, np.uint64), np.array(masses, F32), np.concatenate(intens).astype(F32), [F32(p[0]) for p in plans],
                         [2] * k, np.array(tic, F32), None, None, np.arange(k, dtype=F32) * F32(0.5), None, np.zeros(k, np.uint32))


# ---- the arguments -------------------------------------------------------------------------------------------------------------
def libm_wrong_arguments(per_range=380):
    """arguments on which the platform's log1pf is not the correctly rounded value, from the CPU sweep's own function (a few
    thousand over [2^-12, 2^64]; none if the platform's libm rounds correctly — the floor on their number is test_ln1pf_cpu's)"""
    out = []
    for base in (0x39800000, 0x3C000000, 0x3F800000, 0x40A00000, 0x42000000, 0x44000000, 0x46000000, 0x48000000, 0x4A000000,
                 0x4B800000, 0x5F800000):
        out.append(LN.sweep(base + 12345, base + 12345 + 400000, threads=1, cap=per_range)[3])
    return np.concatenate(out)


def single_arguments():
    """{group: bit patterns} of the summed intensities the single-peak spectra take; MAX_SPECTRA in all"""
    rng = np.random.default_rng(5)
    edges = []
    for e in range(-30, 128):
        b = int(bits_of(np.ldexp(F32(1.0), e)))
        edges += [b - 1, b, b + 1]   # the last value of the binade below, the edge, the first value above it
    groups = {"hard": np.array(LN.HARD_POSITIVE, np.uint32), "libm wrong": libm_wrong_arguments(),
              "binade edges": np.array(edges + [FLT_MAX], np.uint32), "zeros and inf": np.array([0, 0x80000000, INF], np.uint32)}
    used = sum(len(v) for v in groups.values())
    groups["log-uniform fill"] = rng.integers(int(bits_of(F32(2.0 ** -30))), INF, MAX_SPECTRA - used).astype(np.uint32)
    return groups


UNMATCHED = np.array([0x7FC00000, 0xFFC00000, 0xBF800000, 0xC0000000, 0xFF800000, 0xBF000000, 0xB3800000, 0x80000001, 0xBF7FFFFF],
                     np.uint32)   # NaN, -NaN, -1, -2, -inf, -0.5, -2^-24, the smallest negative subnormal, the value above -1


def singles(w, arg_bits):
    """one spectrum per argument: the narrow window of a home peptide, ONE peak on its isolated b ion (even spectra) or y ion (odd).
    Returns (batch, home peptide per spectrum, is-b per spectrum)."""
    plans, pep, is_b = [], [], []
    for i, a in enumerate(arg_bits):
        p, b_ion, y_ion = w.homes[i % len(w.homes)]
        use_b = (i // len(w.homes)) % 2 == 0
        plans.append((holding_precursor(tol_tuple(NARROW), 2, w.db.pep_mono[p]), [(b_ion if use_b else y_ion, int(a))]))
        pep.append(p)
        is_b.append(use_b)
    return make_batch(w, plans), np.array(pep, np.uint32), np.array(is_b)


def single_params(**kw):
    return ScorerParams(**dict(dict(score_type="OpenMSHyperScore", min_matched_peaks=1, report_psms=1, precursor_tol=NARROW,
                                    fragment_tol=FRAGMENT_TOL, max_fragment_charge=1), **kw))


def sums(w, arg_bits):
    """a b peak and a y peak of one home whose f32 sum is the argument: c = f32(t / 4) on the b ion, t - c on the y ion, kept where
    f32(c + (t - c)) == t; and one pair of FLT_MAX whose sum overflows.  Returns (batch, peptides, summed intensity bits)."""
    plans, pep, si = [], [], []
    with np.errstate(all="ignore"):
        for i, t in enumerate(list(f32_of(arg_bits)) + [None]):
            p, b_ion, y_ion = w.homes[i % len(w.homes)]
            c, a = (F32(np.finfo(F32).max),) * 2 if t is None else (F32(t * F32(0.25)), F32(t - F32(t * F32(0.25))))
            if t is not None and (bits_of(F32(c + a)) != bits_of(t) or not c > 0):
                continue
            plans.append((holding_precursor(tol_tuple(NARROW), 2, w.db.pep_mono[p]), [(b_ion, int(bits_of(c))), (y_ion, int(bits_of(a)))]))
            pep.append(p)
            si.append(int(bits_of(F32(c + a))))
    assert si[-1] == INF
    return make_batch(w, plans), np.array(pep, np.uint32), np.array(si, np.uint32)


# ---- ranking pairs -------------------------------------------------------------------------------------------------------------
def ranking_pairs(w, n_each=150):
    """Spectra with TWO candidates of one matched b ion each, under the whole-database window: adjacent f32 intensities x < x+ on
    the isolated b ions of two homes, once as (P: x, Q: x+) and once swapped.  `same`: ln_1p rounds both to one f32 — the
    hyperscores are equal and the order is the tie order, whoever holds which; `different`: the holder of x+ ranks first.
    Half of the x are arguments the platform's log1pf gets wrong (or their lower neighbours).
    Returns (batch, rows): rows[i] = (P, Q, bits on P, bits on Q, same?)."""
    rng = np.random.default_rng(9)
    wrong = libm_wrong_arguments(120)
    cand = np.concatenate([wrong, wrong - 1, rng.integers(int(bits_of(F32(4.0))), int(bits_of(F32(1e7))), 4000).astype(np.uint32)])
    ref_lo, ref_hi = LN.ref_ln1pf(cand), LN.ref_ln1pf(cand + 1)
    same = ref_lo == ref_hi
    lm = LN.libm_log1pf(cand) != ref_lo
    picks = []
    for want_same in (True, False):
        idx = np.flatnonzero(same == want_same)
        from_wrong = idx[lm[idx] | (idx < 2 * len(wrong))][:n_each // 2]
        others = np.setdiff1d(idx, from_wrong)[:n_each - len(from_wrong)]
        picks += [(int(cand[i]), want_same) for i in np.concatenate([from_wrong, others])]
    plans, rows = [], []
    for k, (x, is_same) in enumerate(picks):
        (p, pb, _), (q, qb, _) = w.homes[(2 * k) % len(w.homes)], w.homes[(2 * k + 1) % len(w.homes)]
        for on_p, on_q in ((x, x + 1), (x + 1, x)):
            plans.append((w.middle_mz, [(pb, on_p), (qb, on_q)]))
            rows.append((p, q, on_p, on_q, is_same))
    return make_batch(w, plans), rows


def pair_params(**kw):
    return single_params(**dict(dict(report_psms=2, precursor_tol=world().whole), **kw))


# ---- hundreds of tied candidates: the way into the retry pass -----------------------------------------------------------------------
def tie_arguments():
    """arguments t in [8, 2^24): t - 1 is an f32 and 1 + (t - 1) == t exactly (and from 8 on the home outscores the b1-only candidates
    whichever of its ions is hit: lnfact(0) is 1.0, scoring.rs:171-172)"""
    rng = np.random.default_rng(13)
    lo, hi = int(bits_of(F32(8.0))), int(bits_of(F32(2.0 ** 24)))
    hard = np.array([b for b in LN.HARD_POSITIVE if lo <= b < hi], np.uint32)
    wrong = libm_wrong_arguments(30)
    return np.concatenate([hard, wrong[(wrong >= lo) & (wrong < hi)], rng.integers(lo, hi, 150).astype(np.uint32)])


def ties(w, arg_bits):
    """the whole-database window, a peak of intensity 1 on b1 (EVERY peptide matches it: more candidates than the k-select keeps,
    all with the same score) and a peak of intensity t - 1 on a home's isolated ion: the home ranks first with the summed
    intensity t, and the second reported rank is taken from hundreds of equal hyperscores.  Returns (batch, homes, is-b)."""
    plans, pep, is_b = [], [], []
    for i, t in enumerate(f32_of(arg_bits)):
        p, b_ion, y_ion = w.homes[i % len(w.homes)]
        use_b = i % 2 == 0
        x = F32(t - F32(1.0))
        assert bits_of(F32(F32(1.0) + x)) == bits_of(t)
        plans.append((w.middle_mz, [(w.b1, int(bits_of(F32(1.0)))), (b_ion if use_b else y_ion, int(bits_of(x)))]))
        pep.append(p)
        is_b.append(use_b)
    return make_batch(w, plans), np.array(pep, np.uint32), np.array(is_b)
