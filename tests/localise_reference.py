"""A plain restatement of site localisation (after Beausoleil et al. 2006) — TEST INFRASTRUCTURE.

Straight loops over the spectrum and ion helpers of tests/second_reading.py (the tolerance bounds, the binary search of
select_most_intense_peak, the ion series, the fragment charges, the chimera's peak removal are imported, not copied); the f64
arithmetic with math.lgamma, math.exp and math.log.
"""
import math

import numpy as np

import second_reading as SR

NONE = 0xFFFFFFFF
NO_PEAK = 255
WEIGHTS = (0.5, 0.75, 1.0, 1.0, 1.0, 1.0, 0.75, 0.5, 0.25, 0.25)
f32 = np.float32


def window_of(mass):
    return int(math.floor(f32(mass) / f32(100.0)))


def depth_ranks(masses, intensities):
    """rank[p] = 1 + #{q in p's 100-window: intensity[q] > intensity[p], or equal and q < p}, stored as 11 above 11"""
    ranks = np.zeros(len(masses), dtype=np.uint8)
    wins = np.array([window_of(m) for m in masses], dtype=np.int64)
    it = np.asarray(intensities, dtype=np.float32)
    q = np.arange(len(masses))
    for p in range(len(masses)):  # (every peak against every peak: no use of the order of the masses)
        ahead = (wins == wins[p]) & ((it > it[p]) | ((it == it[p]) & (q < p)))
        ranks[p] = min(1 + int(np.count_nonzero(ahead)), 11)
    return ranks


def min_rank(masses, ranks, center, tol):
    """the smallest rank over the peaks select_most_intense_peak (spectrum.rs:134-159) looks at for `center`; 255: none"""
    lo, hi = SR.bounds(tol, center)
    i, j = SR.binary_search_slice(masses, lo, hi)
    best = NO_PEAK
    for idx in range(i, j):
        if masses[idx] >= lo and masses[idx] <= hi:
            best = min(best, int(ranks[idx]))
    return best


def items(sr, pep, charge):
    """[(ion as f32, fragment charge)] in score_candidate's order (scoring.rs:675-767): kind, ion, charge 1 .. mfc - 1"""
    mfc = SR.max_fragment_charge(sr.p.max_fragment_charge, charge)
    return [(ion, z) for kind in sr.kinds for ion in sr.db.ion_series(pep, kind) for z in range(1, mfc)]


def item_min_ranks(sr, masses, ranks, pep, charge):
    with np.errstate(all="ignore"):
        return [min_rank(masses, ranks, ion / f32(z), sr.fragment_tol) for ion, z in items(sr, pep, charge)]


def counts_of(min_ranks):
    """n[d], d = 1..10"""
    return [sum(1 for m in min_ranks if m <= d) for d in range(1, 11)]


def depth_score(n, N, d):
    """-10 log10 P(X >= n), X ~ Binomial(N, d / 100), by log-sum-exp over ascending k"""
    if n == 0 or N == 0:
        return 0.0
    p = d / 100.0
    ls = [math.lgamma(N + 1) - math.lgamma(k + 1) - math.lgamma(N - k + 1) + k * math.log(p) + (N - k) * math.log(1 - p)
          for k in range(n, N + 1)]
    m = max(ls)
    total = 0.0
    for v in ls:
        total += math.exp(v - m)
    return -10.0 / math.log(10.0) * (m + math.log(total))


def peptide_score(n, N):
    total = 0.0
    for d in range(1, 11):
        total += WEIGHTS[d - 1] * depth_score(n[d - 1], N, d)
    return total / 7.0


def ascore(a, b, Ns):
    """(d*, ascore): the depth with the largest a[d] - b[d], ties to the smallest"""
    if Ns == 0:
        return 1, 0.0
    d_star = 1
    for d in range(2, 11):
        if a[d - 1] - b[d - 1] > a[d_star - 1] - b[d_star - 1]:
            d_star = d
    return d_star, depth_score(a[d_star - 1], Ns, d_star) - depth_score(b[d_star - 1], Ns, d_star)


def localise(sr, masses, intensities, peps, charges):
    """One slot: candidates `peps` at precursor charges `charges` against one spectrum state.  Returns a dict shaped like
    SageLocalisation plus `counts` ([(n[10], N)] per candidate)."""
    ranks = depth_ranks(masses, intensities)
    mrs = [item_min_ranks(sr, masses, ranks, p, z) for p, z in zip(peps, charges)]
    counts = [(counts_of(m), len(m)) for m in mrs]
    out = dict(counts=counts, best=NONE, second=NONE, best_score=0.0, second_score=0.0, ascore=float("nan"), n_site_items=0,
               a=[0] * 10, b=[0] * 10, depth=0)
    if not peps:
        return out
    scores = [peptide_score(n, N) for n, N in counts]
    best = 0
    for j in range(1, len(peps)):
        if scores[j] > scores[best]:
            best = j
    out.update(best=best, best_score=scores[best])
    if len(peps) < 2:
        return out
    second = None
    for j in range(len(peps)):
        if j != best and (second is None or scores[j] > scores[second]):
            second = j
    ia, ib = items(sr, peps[best], charges[best]), items(sr, peps[second], charges[second])
    assert len(ia) == len(ib)
    site = [t for t in range(len(ia)) if f32(ia[t][0]).view(np.uint32) != f32(ib[t][0]).view(np.uint32)]
    a, b = counts_of([mrs[best][t] for t in site]), counts_of([mrs[second][t] for t in site])
    depth, score = ascore(a, b, len(site))
    out.update(second=second, second_score=scores[second], n_site_items=len(site), a=a, b=b, depth=depth, ascore=score)
    return out


def close(got, want, tol=1e-12):
    """an f64 against the restatement, as tests/test_gpu_isomers.py compares one: relative to max(|want|, 1)"""
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= tol * max(abs(want), 1.0)


def assert_slot_equal(got, want, ctx):
    """a SageLocalisation record against localise(): integers for equality, the three f64 to 1e-12"""
    for k in ("best", "second", "n_site_items", "depth"):
        assert int(got[k]) == int(want[k]), f"{ctx}: {k}: device {int(got[k])} vs restatement {int(want[k])}"
    for k in ("a", "b"):
        assert [int(x) for x in got[k]] == list(want[k]), f"{ctx}: {k}: device {list(got[k])} vs restatement {want[k]}"
    for k in ("best_score", "second_score", "ascore"):
        assert close(float(got[k]), float(want[k])), f"{ctx}: {k}: device {float(got[k])!r} vs restatement {float(want[k])!r}"


def assert_counts_equal(got, want, ctx):
    """SageDepthCounts records against localise()['counts']"""
    assert len(got) == len(want), ctx
    for j, (g, (n, N)) in enumerate(zip(got, want)):
        assert [int(x) for x in g["n"]] == n and int(g["n_items"]) == N and int(g["pad"]) == 0, \
            f"{ctx} candidate {j}: device {list(g['n'])} of {int(g['n_items'])} vs restatement {n} of {N}"
