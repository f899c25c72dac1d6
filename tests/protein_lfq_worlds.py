"""Named worlds of the protein roll-up: small inputs, each built to reach one seam of the device code, and each
asserting first that it does (in the style of tests/lfq_trace_worlds.py).  tests/test_protein_lfq_cpu.py runs the host emulation
over them, tests/test_gpu_protein_lfq.py the device; both compare with reference(), the restatement's answer, computed once.

The seams are those of sage_amd/csrc/protein_lfq.hip: a wavefront ranks up to 64 shared rows one per lane, selects by radix over
LDS up to 1 024 rows of a protein and over the columns beyond; the solve kernel keeps n (n + 2) doubles in 64 KB of LDS, that is up
to 89 files, and works in global memory beyond."""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

import protein_lfq_reference as REF

NONE = 0xFFFFFFFF
LANES, LDS_KEYS, LDS_BYTES = 64, 1024, 64 * 1024


@dataclass
class World:
    name: str
    areas: np.ndarray            # [n_rows, n_files] f64
    protein_of_row: np.ndarray   # [n_rows] u32
    n_proteins: int
    min_ratio_count: int = 1
    workspace_mb: Optional[float] = None   # SAGE_HIP_PLFQ_WORKSPACE_MB of the device call
    min_batches: int = 0                   # n_batches of the device call is at least this

    @property
    def n_files(self):
        return self.areas.shape[1]


def present(a):
    return (a > 0) & np.isfinite(a)


def shared_counts(w: World, protein: int):
    """{(j, k): rows of the protein present in both files}"""
    m = present(w.areas[w.protein_of_row == protein])
    return {(j, k): int((m[:, j] & m[:, k]).sum()) for j in range(w.n_files) for k in range(j + 1, w.n_files)}


def draw(rng, rows, files, missing):
    a = np.exp(rng.normal(14.0, 2.0, (rows, files)))
    a[rng.random((rows, files)) < missing] = 0.0
    return a


def _rows_world(rows):
    """one protein of `rows` rows over 3 files (files 0 and 1 complete, so their pair shares every row; file 2 sparse) and a
    second protein of 2 rows"""
    rng = np.random.default_rng(1000 + rows)
    a = draw(rng, rows + 2, 3, 0.0)
    sparse = rng.random(rows) < (0.5 if rows < 1000 else 0.97)
    a[:rows, 2][sparse] = 0.0
    w = World(f"rows_{rows}", a, np.array([0] * rows + [1, 1], np.uint32), 2)
    c = shared_counts(w, 0)
    assert c[(0, 1)] == rows
    if rows == 129:
        assert LANES < c[(0, 1)] <= LDS_KEYS        # radix select over LDS
    if rows == 1500:
        assert c[(0, 1)] > LDS_KEYS                 # radix select over the columns
        assert 0 < c[(0, 2)] <= LANES               # few shared rows of a protein too long for LDS
    return w


def _files_world(files):
    rng = np.random.default_rng(2000 + files)
    a = draw(rng, 9, files, 0.3)
    w = World(f"files_{files}", a, np.array([0] * 4 + [1] * 5, np.uint32), 2)
    fits = files * (files + 2) * 8 <= LDS_BYTES
    assert fits == (files <= 89)
    if files == 130:
        assert not fits                             # the matrix in the global workspace
    if files == 1:
        assert not shared_counts(w, 0)              # no pair
    return w


def _threshold_world(mc):
    """files 0 and 1 share exactly mc rows, files 1 and 2 one fewer; file 2 ends up isolated"""
    rng = np.random.default_rng(3000 + mc)
    a = draw(rng, 2 * mc - 1, 3, 0.0)
    a[:mc, 2] = 0.0
    a[mc:, 0] = 0.0
    w = World(f"min_ratio_count_{mc}", a, np.zeros(2 * mc - 1, np.uint32), 1, min_ratio_count=mc)
    c = shared_counts(w, 0)
    assert c[(0, 1)] == mc and c[(1, 2)] == mc - 1 and c[(0, 2)] == 0
    return w


def _odd_even():
    rng = np.random.default_rng(4)
    a = draw(rng, 9, 3, 0.0)
    w = World("odd_even", a, np.array([0] * 4 + [1] * 5, np.uint32), 2)
    assert shared_counts(w, 0)[(0, 1)] == 4 and shared_counts(w, 1)[(0, 1)] == 5
    return w


def _ties():
    rng = np.random.default_rng(5)
    base = draw(rng, 2, 4, 0.0)
    a = np.concatenate([base[[0]]] * 4 + [base[[1]]] * 3 + [base[[0]] * 2.0, draw(rng, 2, 4, 0.0)])  # identical rows; a row doubled
    w = World("ties", a, np.zeros(len(a), np.uint32), 1)
    d = np.log(a[:, 0]) - np.log(a[:, 1])
    assert len(np.unique(d[:4])) == 1 and len(a) == 10
    return w


def _absent_file():
    rng = np.random.default_rng(6)
    a = draw(rng, 10, 4, 0.1)
    a[:5, 2] = 0.0
    w = World("absent_file", a, np.array([0] * 5 + [1] * 5, np.uint32), 2)
    assert not present(a[:5, 2]).any() and present(a[5:, 2]).any()
    return w


def _two_components():
    rng = np.random.default_rng(7)
    a = draw(rng, 8, 5, 0.0)
    a[:4, 2:] = 0.0
    a[4:, :2] = 0.0
    w = World("two_components", a, np.zeros(8, np.uint32), 1)
    c = shared_counts(w, 0)
    assert all((c[(j, k)] > 0) == ((j < 2) == (k < 2)) for (j, k) in c)
    return w


def _isolated_file():
    rng = np.random.default_rng(8)
    a = draw(rng, 6, 3, 0.0)
    a[:4, 2] = 0.0
    a[4:, :2] = 0.0
    w = World("isolated_file", a, np.zeros(6, np.uint32), 1)
    c = shared_counts(w, 0)
    assert c[(0, 2)] == 0 and c[(1, 2)] == 0 and present(a[:, 2]).sum() == 2
    return w


def _all_missing():
    rng = np.random.default_rng(9)
    a = draw(rng, 6, 3, 0.0)
    a[:3] = 0.0
    return World("all_missing", a, np.array([0] * 3 + [1] * 3, np.uint32), 2)


def _special_areas():
    a = np.array([[5e-324, 1e300, 0.0, 7.0],
                  [1e300, 5e-324, -1.0, 9.0],
                  [np.nan, 3.0, np.inf, 5e-324],
                  [2.0, np.inf, 1e300, np.nan],
                  [5e-324, 5e-324, 1e300, 1e300],
                  [-np.inf, 4.0, 6.0, -0.0]])
    w = World("special_areas", a, np.zeros(6, np.uint32), 1)
    assert present(a).sum() == 16
    return w


def _shuffled():
    rng = np.random.default_rng(10)
    rows = 60
    a = draw(rng, rows, 4, 0.3)
    p = rng.integers(0, 7, rows).astype(np.uint32)
    p[rng.random(rows) < 0.2] = NONE
    p[0], p[1] = 6, 0   # the ids do not appear in ascending order
    w = World("shuffled", a, p, 7)
    assert (p == NONE).sum() > 3 and (np.diff(p[p != NONE].astype(np.int64)) < 0).any()
    return w


def _batches():
    rng = np.random.default_rng(11)
    a = draw(rng, 200, 5, 0.35)
    p = rng.integers(0, 40, 200).astype(np.uint32)
    # 10 pairs * 12 bytes + 5 files * 32 bytes + 8 = 288 bytes per protein: 14 proteins in 0.004 MB, three batches
    return World("batches", a, p, 40, workspace_mb=0.004, min_batches=3)


def _zero_rows():
    return World("zero_rows", np.zeros((0, 3)), np.zeros(0, np.uint32), 2)


def _zero_proteins():
    return World("zero_proteins", np.ones((2, 3)), np.full(2, NONE, np.uint32), 0)


def _build():
    ws = [_rows_world(r) for r in (1, 2, 3, 63, 64, 65, 129, 1500)]
    ws += [_files_world(f) for f in (1, 2, 3, 5, 64, 65, 130)]
    ws += [_threshold_world(mc) for mc in (1, 2, 3)]
    ws += [_odd_even(), _ties(), _absent_file(), _two_components(), _isolated_file(), _all_missing(), _special_areas(), _shuffled(),
           _batches(), _zero_rows(), _zero_proteins()]
    return {w.name: w for w in ws}


WORLDS = _build()
NAMES = list(WORLDS)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """the restatement's answer for a world; shared by every test, never changed"""
    w = WORLDS[name]
    return REF.protein_lfq(w.areas.tolist(), w.protein_of_row.tolist(), w.n_proteins, w.min_ratio_count, n_files=w.n_files)


def random_world(seed: int) -> World:
    """<= 12 rows, <= 9 files, 40 % missing, up to 3 proteins"""
    rng = np.random.default_rng(seed)
    rows, files, proteins = int(rng.integers(1, 13)), int(rng.integers(1, 10)), int(rng.integers(1, 4))
    return World(f"random_{seed}", draw(rng, rows, files, 0.4), rng.integers(0, proteins, rows).astype(np.uint32), proteins,
                 min_ratio_count=int(rng.integers(1, 3)))


def assert_equal(got: dict, want: dict, what: str, pair_tables: bool = True):
    """got: arrays [n_proteins, ...] of an implementation; want: reference().  Bit for bit (NaN positions included) except the
    intensity, which is within 1 ulp of the correctly rounded exp."""
    def same(a, b, key):
        a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, key, "NaN positions")
        ok = ~np.isnan(a)
        bad = np.flatnonzero(a[ok].view(np.uint64) != b[ok].view(np.uint64))
        assert len(bad) == 0, (what, key, len(bad), a[ok][bad[:3]].tolist(), b[ok][bad[:3]].tolist())

    for key in ("component", "n_rows_used", "n_components") + (("pair_count",) if pair_tables else ()):
        a, b = np.asarray(got[key], np.int64).reshape(-1), np.asarray(want[key], np.int64).reshape(-1)
        assert np.array_equal(a, b), (what, key)
    same(got["log_abundance"], want["log_abundance"], "log_abundance")
    if pair_tables:
        same(got["pair_median"], want["pair_median"], "pair_median")
    gi, wi = np.asarray(got["intensity"], np.float64).reshape(-1), np.asarray(want["intensity"], np.float64).reshape(-1)
    assert gi.shape == wi.shape
    for g, x in zip(gi.tolist(), wi.tolist()):
        if x == 0.0 or x == float("inf"):
            assert g == x or (x == float("inf") and REF.ulp_distance(g, x) <= 1), (what, "intensity", g, x)
        else:
            assert REF.ulp_distance(g, x) <= 1, (what, "intensity", g, x)
