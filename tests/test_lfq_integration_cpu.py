"""A condition of tests/test_gpu_lfq_integration.py, checked without a GPU: the drawn cases' decisions do not hang on the last
bits of an angle.

The device's acos may lie a few units in the last place from libm's, so a case whose best bin or bounds flip under such a
difference would fail on the device without any bug.  Every (case, peak_scoring, spectral_angle) combination is integrated again
by tests/lfq_reference.py with its acos moved by ACOS_ULPS units — every value up, every value down, alternating by element —
and must keep has_peak, the warps, the best bin and both bounds.  The combinations that do not are lfq_traces.FRAGILE, by
name; the device is compared on those for matrix and warps only.  The list is capped: at least 90 % of all combinations and at
least 6 of each case's 8 must be robust.  A case below the cap needs another drawing, not another cap."""
import numpy as np
import pytest

import lfq_reference as R
import lfq_traces as T

PATTERNS = ("up", "down", "alternating")


def nudged_acos(pattern, ulps=T.ACOS_ULPS):
    plain = R._acos

    def acos(x):
        a = np.asarray(plain(x), dtype=np.float64)
        up, down = a.copy(), a.copy()
        for _ in range(ulps):
            up, down = np.nextafter(up, np.inf), np.nextafter(down, -np.inf)
        if pattern == "up":
            return up
        if pattern == "down":
            return down
        even = (np.arange(a.size).reshape(a.shape) % 2) == 0
        return np.where(even, up, down)
    return acos


def decisions(world, scoring, thr):
    out = []
    st = R.default_settings(peak_scoring=scoring, spectral_angle=thr)
    for combine in sorted(world["grids"]):
        for key in sorted(world["grids"][combine]):
            r = R.integrate(world["grids"][combine][key], st)
            out.append((combine, key, r["peak"], r["warps"], r.get("rt"), r.get("left"), r.get("right")))
    return out


@pytest.fixture(scope="module")
def fragile():
    db = T.database()
    found = set()
    for name in T.CASES:
        world = T.case(db, name)
        for scoring in R.SCORING:
            for thr in T.THRESHOLDS:
                plain = decisions(world, scoring, thr)
                for pattern in PATTERNS:
                    saved = R._acos
                    R._acos = nudged_acos(pattern)
                    try:
                        moved = decisions(world, scoring, thr)
                    finally:
                        R._acos = saved
                    if moved != plain:
                        found.add((name, scoring, thr))
    return found


def test_nudge_moves_the_angle():
    x = np.array([0.0, 0.5, 1.0, np.nan, 2.0])
    with np.errstate(invalid="ignore"):
        plain = R._acos(x)
    for pattern, sign in (("up", [1, 1, 1]), ("down", [-1, -1, -1]), ("alternating", [1, -1, 1])):
        with np.errstate(invalid="ignore"):
            moved = nudged_acos(pattern)(x)
        assert np.isnan(moved[3:]).all() and np.sign(moved[:3] - plain[:3]).tolist() == sign
        assert np.all(np.abs(moved[:2] - plain[:2]) == T.ACOS_ULPS * np.spacing(plain[:2]))


def test_nudges_flip_a_decision_that_hangs_on_an_angle():
    """the check can fail: with the threshold set exactly on the spectral value of the bin that stopped a walk, the walk's end
    hangs on the last bits of acos, and a nudge moves it"""
    world = T.case(T.database(), "threshold_stop")
    grid = next(iter(world["grids"][True].values()))
    st = R.default_settings(peak_scoring="Intensity", spectral_angle=0.70)
    right = R.integrate(grid, st)["right"]
    # the bin that stopped the walk, now exactly on the threshold.  (An angle close to 1.0 would not do: there acos is small
    # and 8 of its ulps vanish in the rounding of 1 - 2 acos / pi.)
    on_the_edge = float(T.stages(grid, st)["spectral"][right])
    assert 0.2 < on_the_edge < 0.70
    st = dict(st, spectral_angle=on_the_edge)
    pick = lambda r: (r["peak"], r.get("rt"), r.get("left"), r.get("right"))
    plain = pick(R.integrate(grid, st))
    moved = set()
    for pattern in PATTERNS:
        saved = R._acos
        R._acos = nudged_acos(pattern)
        try:
            moved.add(pick(R.integrate(grid, st)))
        finally:
            R._acos = saved
    assert plain[0] and moved != {plain}, (plain, moved)


def test_fragile_list_is_what_the_nudges_find(fragile):
    assert fragile == set(T.FRAGILE), (sorted(fragile - set(T.FRAGILE)), sorted(set(T.FRAGILE) - fragile))


def test_fragile_list_is_within_its_cap(fragile):
    total = len(T.CASES) * len(R.SCORING) * len(T.THRESHOLDS)
    assert total - len(fragile) >= 0.9 * total, f"{total - len(fragile)} of {total} combinations are robust"
    for name in T.CASES:
        n = sum(1 for f in fragile if f[0] == name)
        assert 8 - n >= 6, f"{name}: {8 - n} of 8 combinations are robust"
