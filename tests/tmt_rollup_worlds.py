"""Named worlds of the TMT roll-up: small inputs, each built to reach one seam of the device code, and each asserting
first that it does (in the style of tests/protein_lfq_worlds.py).  tests/test_tmt_rollup_cpu.py runs the host emulation over them,
tests/test_gpu_tmt_rollup.py the device; both compare with reference(), the restatement's answer, computed once per world and
(summary, normalise) pair.

The seams are those of sage_amd/csrc/tmt_rollup.hip: column sums in blocks of 1 024 input rows; a wavefront walks the channels in
slabs of 64; it ranks up to 64 keys one per lane, selects by radix over LDS up to 1 024 used rows of a group and over the column in
global memory beyond."""
import functools
from dataclasses import dataclass

import numpy as np

import tmt_rollup_reference as REF

NONE = 0xFFFFFFFF
LANES, LDS_KEYS, BLOCK_ROWS = 64, 1024, 1024
PAIRS = [(s, n) for s in ("Sum", "Median") for n in ("Total", "None")]
TINY = np.float32(1e-45)  # the smallest subnormal f32


@dataclass
class World:
    name: str
    intensity: np.ndarray        # [n_rows, n_labels] f32
    group_of_row: np.ndarray     # [n_rows] u32
    n_groups: int
    min_present: int = 1
    long_groups: int = 0         # n_long_groups of the device's Median call is at least this

    @property
    def n_labels(self):
        return self.intensity.shape[1]


def present(a):
    a = np.asarray(a, np.float64)
    return (a > 0) & (a < np.inf)


def used_rows(w: World):
    return (w.group_of_row != NONE) & (present(w.intensity).sum(axis=1) >= max(w.min_present, 1))


def used_per_group(w: World):
    return np.bincount(w.group_of_row[used_rows(w)].astype(np.int64), minlength=w.n_groups)


def draw(rng, rows, labels, missing):
    a = np.exp(rng.normal(10.0, 2.0, (rows, labels))).astype(np.float32)
    a[rng.random((rows, labels)) < missing] = 0.0
    return a


def _labels_world(labels):
    rng = np.random.default_rng(100 + labels)
    w = World(f"labels_{labels}", draw(rng, 9, labels, 0.3), np.array([0] * 4 + [1] * 5, np.uint32), 2)
    assert (labels + LANES - 1) // LANES == {1: 1, 18: 1, 64: 1, 65: 2, 130: 3}[labels]   # the slabs a wavefront walks
    assert used_per_group(w).min() >= 1
    return w


def _group_sizes():
    """groups of 0, 1, 2, 63, 64 and 65 used rows (and one row each that min_present leaves out)"""
    rng = np.random.default_rng(200)
    sizes = [0, 1, 2, 63, 64, 65]
    ids = np.concatenate([np.full(s + 1, g, np.uint32) for g, s in enumerate(sizes)])
    a = draw(rng, len(ids), 3, 0.0)
    first = np.concatenate([[0], np.cumsum([s + 1 for s in sizes])[:-1]])
    a[first, 1:] = 0.0                      # the first row of every group keeps one cell: not used at min_present 2
    perm = rng.permutation(len(ids))
    w = World("group_sizes", a[perm], ids[perm], len(sizes), min_present=2)
    assert used_per_group(w).tolist() == sizes
    return w


def _long_group():
    rng = np.random.default_rng(300)
    rows = LDS_KEYS + 76
    ids = np.zeros(rows + 5, np.uint32)
    ids[rng.choice(rows + 5, 5, replace=False)] = 1
    a = draw(rng, rows + 5, 2, 0.0)
    a[rng.random(rows + 5) < 0.96, 1] = 0.0     # few cells of a group too long for LDS in channel 1
    w = World("long_group", a, ids, 2, long_groups=1)
    assert used_per_group(w)[0] > LDS_KEYS
    n1 = int(present(a[ids == 0, 1]).sum())
    assert 0 < n1 <= LANES
    return w


def _interleaved():
    rng = np.random.default_rng(400)
    rows = 80
    g = rng.integers(0, 9, rows).astype(np.uint32)
    g[g == 4] = 3                               # group 4 is empty
    g[rng.random(rows) < 0.2] = NONE
    g[0], g[1] = 8, 0                           # the ids do not appear in ascending order
    w = World("interleaved", draw(rng, rows, 5, 0.3), g, 10)
    n = used_per_group(w)
    assert n[4] == 0 and n[9] == 0 and (g == NONE).sum() > 3 and (np.diff(g[g != NONE].astype(np.int64)) < 0).any()
    return w


def _special_cells():
    a = np.array([[np.nan, 3.0, np.inf, TINY],
                  [2.0, -1.0, 7.0, 0.0],
                  [TINY, TINY, -0.0, 5.0],
                  [-np.inf, 4.0, 6.0, np.nan],
                  [3.4e38, 1.0, TINY, 3.4e38],
                  [np.nan, np.inf, -1.0, -0.0]], np.float32)
    w = World("special_cells", a, np.array([0, 0, 0, 1, 1, 1], np.uint32), 2)
    assert present(a).sum() == 13 and TINY > 0 and np.float32(TINY / 2) == 0
    assert used_rows(w).tolist() == [True] * 5 + [False]   # the last row has no present cell
    return w


def _min_present():
    rng = np.random.default_rng(500)
    rows = BLOCK_ROWS + 6
    a = draw(rng, rows, 3, 0.0)
    thin = [0, 500, BLOCK_ROWS - 1, BLOCK_ROWS, rows - 1]
    a[thin, :2] = 0.0                           # one cell left: dropped, on both sides of the block seam too
    w = World("min_present", a, rng.integers(0, 4, rows).astype(np.uint32), 4, min_present=2)
    u = used_rows(w)
    assert not u[thin].any() and u.sum() == rows - len(thin)
    return w


def _rows_world(rows):
    rng = np.random.default_rng(600 + rows)
    w = World(f"rows_{rows}", draw(rng, rows, 2, 0.2), rng.integers(0, 3, rows).astype(np.uint32), 3)
    assert (rows + BLOCK_ROWS - 1) // BLOCK_ROWS == {1023: 1, 1024: 1, 1025: 2, 2049: 3}[rows]
    return w


def _absent_channel():
    rng = np.random.default_rng(700)
    a = draw(rng, 12, 4, 0.1)
    a[:, 2] = 0.0
    w = World("absent_channel", a, np.array([0] * 6 + [1] * 6, np.uint32), 2)
    assert not present(a[:, 2]).any() and present(a[:, 3]).any()
    return w


def _ties_even():
    rng = np.random.default_rng(800)
    base = draw(rng, 2, 4, 0.0)
    a = np.concatenate([base[[0]]] * 4 + [base[[1]]] * 3 + [base[[0]] * np.float32(2.0), draw(rng, 2, 4, 0.0)])   # identical rows; one doubled
    w = World("ties_even", a, np.array([0] * 10, np.uint32), 1)
    assert len(a) == 10 and (a[:4] == a[0]).all()       # an even count, its middle pair among ties
    return w


def _order_of_addition():
    """2^53, 1, 1: in this order the sum stays 2^53, in any order that adds the ones first it is 2^53 + 2.  Channel 0: three rows of
    group 0 inside block 0.  Channel 2: three rows of group 1 across the seam of blocks 0 and 1, so the group's sum (in row order) is
    2^53 and the column sum (block by block) 2^53 + 2.  Channel 1 holds ordinary values."""
    rng = np.random.default_rng(900)
    rows = BLOCK_ROWS + 4
    a = np.zeros((rows, 3), np.float32)
    g = np.full(rows, NONE, np.uint32)
    big = np.float32(2.0 ** 53)
    for group, at, ch in ((0, [10, 11, 12], 0), (1, [BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1], 2)):
        g[at] = group
        a[at, ch] = [big, 1.0, 1.0]
        a[at, 1] = draw(rng, 3, 1, 0.0)[:, 0]
    w = World("order_of_addition", a, g, 2)
    fwd = REF.tmt_rollup(a.tolist(), g.tolist(), 2, 1, "None", "Sum")
    rev = REF.tmt_rollup(a.tolist(), g.tolist(), 2, 1, "None", "Sum", descending=True)
    assert fwd["abundance"][0][0] == 2.0 ** 53 and rev["abundance"][0][0] == 2.0 ** 53 + 2.0
    assert fwd["abundance"][1][2] == 2.0 ** 53 and rev["abundance"][1][2] == 2.0 ** 53 + 2.0
    assert fwd["column_sum"][0] == 2.0 ** 53 and rev["column_sum"][0] == 2.0 ** 53 + 2.0
    assert fwd["column_sum"][2] == 2.0 ** 53 + 2.0      # block by block: not the sum in plain row order
    tot_f = REF.tmt_rollup(a.tolist(), g.tolist(), 2, 1, "Total", "Sum")
    tot_r = REF.tmt_rollup(a.tolist(), g.tolist(), 2, 1, "Total", "Sum", descending=True)
    assert [REF.bits(x) for x in tot_f["factor"]] != [REF.bits(x) for x in tot_r["factor"]]
    return w


def _all_ignored():
    return World("all_ignored", np.ones((3, 2), np.float32), np.full(3, NONE, np.uint32), 2)


def _no_used_row():
    w = World("no_used_row", np.array([[1.0, 0.0], [0.0, 2.0]], np.float32), np.array([0, 1], np.uint32), 2, min_present=2)
    assert not used_rows(w).any()
    return w


def _zero_rows():
    return World("zero_rows", np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), 2)


def _zero_groups():
    return World("zero_groups", np.ones((2, 3), np.float32), np.full(2, NONE, np.uint32), 0)


def _build():
    ws = [_labels_world(n) for n in (1, 18, 64, 65, 130)]
    ws += [_group_sizes(), _long_group(), _interleaved(), _special_cells(), _min_present()]
    ws += [_rows_world(r) for r in (1023, 1024, 1025, 2049)]
    ws += [_absent_channel(), _ties_even(), _order_of_addition(), _all_ignored(), _no_used_row(), _zero_rows(), _zero_groups()]
    return {w.name: w for w in ws}


WORLDS = _build()
NAMES = list(WORLDS)


def restate(w: World, summary: str, normalise: str):
    return REF.tmt_rollup(w.intensity.tolist(), w.group_of_row.tolist(), w.n_groups, w.min_present, normalise, summary, n_labels=w.n_labels)


@functools.lru_cache(maxsize=None)
def reference(name: str, summary: str, normalise: str):
    """the restatement's answer for a world; shared by every test, never changed"""
    return restate(WORLDS[name], summary, normalise)


def random_world(seed: int) -> World:
    """<= 12 rows, <= 9 channels, 40 % missing, up to 3 groups, some rows ignored"""
    rng = np.random.default_rng(seed)
    rows, labels, groups = int(rng.integers(1, 13)), int(rng.integers(1, 10)), int(rng.integers(1, 4))
    g = rng.integers(0, groups, rows).astype(np.uint32)
    g[rng.random(rows) < 0.15] = NONE
    return World(f"random_{seed}", draw(rng, rows, labels, 0.4), g, groups, min_present=int(rng.integers(0, 4)))


def assert_equal(got: dict, want: dict, what, summary: str):
    """got: arrays of an implementation; want: reference().  Bit for bit (NaN positions included), except Median's abundance, which is
    within 1 ulp of the correctly rounded exp."""
    def same(key):
        a, b = np.asarray(got[key], np.float64).reshape(-1), np.asarray(want[key], np.float64).reshape(-1)
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, key, "NaN positions")
        ok = ~np.isnan(a)
        bad = np.flatnonzero(a[ok].view(np.uint64) != b[ok].view(np.uint64))
        assert len(bad) == 0, (what, key, len(bad), a[ok][bad[:3]].tolist(), b[ok][bad[:3]].tolist())

    for key in ("n_cells", "n_rows_used"):
        a, b = np.asarray(got[key], np.int64).reshape(-1), np.asarray(want[key], np.int64).reshape(-1)
        assert np.array_equal(a, b), (what, key)
    assert int(got["n_used_rows"]) == int(want["n_used_rows"]), (what, "n_used_rows")
    for key in ("log_abundance", "factor", "column_sum"):
        same(key)
    if summary == "Sum":
        same("abundance")
        return
    ga, wa = np.asarray(got["abundance"], np.float64).reshape(-1), np.asarray(want["abundance"], np.float64).reshape(-1)
    assert ga.shape == wa.shape
    for g, x in zip(ga.tolist(), wa.tolist()):
        if x == 0.0:
            assert g == 0.0, (what, "abundance", g, x)
        else:
            assert REF.ulp_distance(g, x) <= 1, (what, "abundance", g, x)
