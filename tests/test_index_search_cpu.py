"""The search worlds over the hand-built index cases (tests/index_search_worlds.py) on the CPU: every world's census holds, and
the C++ oracle — over its own paged index, with bucket seams inside these databases' tie runs — equals the second, index-free
reading (tests/second_reading.py) on the aimed spectra: preliminary lists with heap order, integer and f32 Feature fields bit for
bit, f64 fields to 1e-12.  Only then does tests/test_gpu_index_search.py hold the device to the oracle on the same worlds.

The readers' shared arithmetic (sage_amd/csrc/core.h) meets the same aimed windows here through the host emulation: the position
tables' cells (probe and tile kernels), the window searches of the stream variant, the rescoring kernels' peak table."""
import json

import numpy as np
import pytest

import index_search_worlds as W
import second_reading as SR
from test_core_emulation import emu, fp  # noqa: F401  (the fixture that builds tests/hostemu)
from test_scoring_second_reading import hold_oracle_to_second_reading


@pytest.mark.parametrize("name", W.NAMES)
def test_census(name):
    figures = W.census(W.world(name))
    print(json.dumps(figures))
    with open(W.CENSUS_FILE) as f:
        filed = {c["world"]: c for c in json.load(f)}
    assert filed[name] == json.loads(json.dumps(figures)), "profiles/index_search_census.json is not this world's census (python tests/index_search_worlds.py)"


class _Arrays:
    """hold_oracle_to_second_reading asks the oracle for its peptide arrays and a DatabaseParameters for kinds and min_ion_index"""

    def __init__(self, w):
        self.w = w
        self.ion_kinds = [k for k in ("a", "b", "c", "x", "y", "z") if W.L.ION_KINDS[k] in w.kinds]
        self.min_ion_index = w.min_ion_index


@pytest.mark.parametrize("name", W.NAMES)
def test_oracle_equals_second_reading(name):
    w = W.world(name)
    batch = w.batch if len(w.second_reading_spectra) == w.batch.n else w.batch.subset(w.second_reading_spectra)
    if name == "seam_large_4133":
        assert batch.n >= 8
    dbp = _Arrays(w)
    assert [W.L.ION_KINDS[k] for k in dbp.ion_kinds] == w.kinds
    a = w.oracle.arrays()
    for k, v in W.peptide_arrays(w).items():  # (the oracle holds the list the second reading is given)
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), (name, k)
    for k, params in enumerate(w.settings):
        hold_oracle_to_second_reading(w.oracle, dbp, params, batch, context=f"{name}, setting {k}")


@pytest.mark.parametrize("name", [n for n in W.NAMES if n.startswith(("cell_edges", "signs"))])
def test_aimed_windows_through_the_position_tables(name, emu):
    """The aimed bounds of the cell-edge and sign worlds — windows that end on a stored m/z that is a cell's edge, start inside cell
    0's negative run, or lie in and beyond the last cell — through core.h's lut_cells / lut_entry on the CPU (tests/hostemu): the
    run a window reads misses no entry of the window, in the 1/32 and the 1/256 table, for every tile of the case's geometry."""
    import ctypes as C
    w = W.world(name)
    lo, hi = [], []
    for p in w.settings:
        for i in range(w.batch.n):
            for m in w.batch.masses[int(w.batch.peak_off[i]):int(w.batch.peak_off[i + 1])]:
                for c in W.fragment_charges(p, int(w.batch.precursor_charge[i])):
                    a, b = SR.bounds(W.tol_tuple(p.fragment_tol), np.float32(m) * np.float32(c))
                    lo.append(a)
                    hi.append(b)
    lo, hi = np.array(lo, np.float32), np.array(hi, np.float32)
    assert len(lo) > 500
    beyond = 0
    for shift, scale in zip(W.geometry(w.env), (32.0, 256.0)):
        copy, toff, stride = w.ref.tile_copy(shift)["fragment_mz"], w.ref.tile_offsets(shift), w.ref.stride(scale)
        beyond += int((hi.astype(np.float64) * scale >= stride - 1).sum())
        for t in range(len(toff) - 1):
            mz = np.ascontiguousarray(copy[toff[t]:toff[t + 1]])
            run = C.c_uint64()
            assert emu.emu_lut_windows(fp(mz), len(mz), scale, stride, fp(lo), fp(hi), len(lo), C.byref(run)) == 0, (name, shift, t)
            nonempty = C.c_uint64()
            assert emu.emu_succinct_lut_mismatches(fp(mz), len(mz), scale, stride, 7, C.byref(nonempty)) == 0
    assert beyond > 0, "a window whose hi lies beyond the table"


@pytest.mark.parametrize("name", [n for n in W.NAMES if n.startswith(("signs", "cell_edges_top_k32", "lengths_abcxyz", "termini"))])
def test_rescoring_lookups_through_the_peak_table(name, emu):
    """The rescoring kernels' peak lookup (core.h: select_peak_lut over peak_lut_entry's table) against select_most_intense_peak,
    for every ion of the ion table at fragment charges 1 and 2 on every spectrum of the world — negative ions and negative peaks,
    an ion of exactly 0.0, windows that end on a peak."""
    w = W.world(name)
    ions = np.unique(w.ref.ions)
    assert len(ions)
    kind = {"ppm": 0, "pct": 1, "da": 2}
    n = found = negative = 0
    for p in w.settings:
        k, lo, hi = W.tol_tuple(p.fragment_tol)
        for i in range(w.batch.n):
            a, b = int(w.batch.peak_off[i]), int(w.batch.peak_off[i + 1])
            m, it = np.ascontiguousarray(w.batch.masses[a:b]), np.ascontiguousarray(w.batch.intensities[a:b])
            for c in W.fragment_charges(p, int(w.batch.precursor_charge[i])):
                for ion in (ions if len(ions) <= 400 else ions[:: len(ions) // 400]):
                    centre = np.float32(ion) / np.float32(c)
                    want = emu.emu_select_peak(fp(m), fp(it), len(m), centre, kind[k], lo, hi, 0)
                    got = emu.emu_select_peak_lut(fp(m), fp(it), len(m), centre, kind[k], lo, hi)
                    assert got == want, f"{name}: ion {ion!r} / {c}, spectrum {i}: peak {got} through the table, {want} by the search"
                    n += 1
                    found += want >= 0
                    negative += want >= 0 and m[want] < 0
    assert found > 0, (n, found)
    if name.startswith("signs"):
        assert negative > 0, "a negative peak matched by a negative ion"


@pytest.mark.parametrize("name", ["signs_by", "cell_edges_top_k256", "ties", "empty_middle", "termini_min0"])
def test_stream_counts_through_the_window_searches(name, emu):
    """The stream variant counts, per stored entry, the windows of a spectrum that hold it (core.h: count_windows_scan where the
    windows are not sorted, count_windows_sorted / _lockstep where they are).  Every variant against a plain count, for the aimed
    entries and their neighbours in the index: a window ends exactly on them."""
    w = W.world(name)
    s = w.ref.sorted_entries()["fragment_mz"]
    aimed = np.array([e for _, e in w.aimed], np.float32)
    frags = np.unique(np.concatenate([aimed, s[:: max(1, len(s) // 200)], s[np.clip(np.searchsorted(s, aimed) + 1, 0, len(s) - 1)]]))
    on_an_end = 0
    for p in w.settings:
        tol = W.tol_tuple(p.fragment_tol)
        for i in range(w.batch.n):
            m = w.batch.masses[int(w.batch.peak_off[i]):int(w.batch.peak_off[i + 1])]
            for c in W.fragment_charges(p, int(w.batch.precursor_charge[i])):
                with np.errstate(all="ignore"):
                    b = [SR.bounds(tol, np.float32(x) * np.float32(c)) for x in m]
                lo, hi = np.array([x[0] for x in b], np.float32), np.array([x[1] for x in b], np.float32)
                if not len(lo):
                    continue
                ascending = (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all() and (lo <= hi).all()
                for f in frags:
                    want = int(((lo <= f) & (f <= hi)).sum())
                    on_an_end += int(((lo == f) | (hi == f)).sum())
                    for variant in ((0, 1, 2) if ascending else (0,)):
                        assert emu.emu_count_windows(fp(lo), fp(hi), len(lo), f, variant) == want, (name, variant, f)
    assert on_an_end > 20
