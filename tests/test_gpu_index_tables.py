"""Every table sage_hip_db_create derives in HBM (index_build.hip's kernels, capi_db.hip's host branch), read back through
sage_hip_debug_db_layout / sage_hip_debug_db_table and compared entry for entry, cell for cell and bit for bit with the numpy
restatement of tests/index_reference.py — which tests/test_index_reference_cpu.py anchors to the oracle.  No tolerance anywhere:
every step is the reference's f32 arithmetic or integer work.

The PSM-level tests (test_gpu_parity.py::test_index_built_on_device, test_gpu_config_scale.py) notice a wrong ion or a misplaced
entry only if a peak of a sampled spectrum lands on it; these look at the index itself.  Databases: the four fuzz settings
(test_gpu_fuzz.py::WORLDS) under three table geometries, and the hand-built lists of tests/index_cases.py — tile seams, an empty
tile, every branch of the keep rule, all N-terminal forms and odd residues under all six kinds, negative and zero m/z, m/z on the
cells' edges, ties inside and across tiles, the sort's and scan's small and large paths, the empty database.  Routes: the index
generated on the device from the peptide list, and the host-built one (the device still builds the small-tile copy, its
succinct table, the peptide-mass table and the ion range)."""
import numpy as np
import pytest

from index_cases import HAND_BUILT
from index_reference import IndexReference, decode, succinct
from sage_amd.api import DatabaseParameters, DeviceDatabase
from sage_amd.synthetic import synthetic_fasta
from test_gpu_fuzz import ORDER, WORLDS

pytestmark = pytest.mark.gpu

TABLES = ("ions", "ion_off", "pm_off", "pep_info", "pep_mono", "pep_lut", "pm_frag", "tm_frag", "tm2_frag", "tm_lut", "tm2_l1", "tm2_pos")
ENV = ("SAGE_HIP_TILE_SHIFT", "SAGE_HIP_TILE2_SHIFT", "SAGE_HIP_LUT2_SCALE", "SAGE_HIP_KEEP_PM_FRAG", "SAGE_HIP_NO_PEP_LUT")
GEOMETRIES = {"defaults": {}, "t6_s8": {"SAGE_HIP_TILE2_SHIFT": "6", "SAGE_HIP_LUT2_SCALE": "8"},
              "t9_s256": {"SAGE_HIP_TILE2_SHIFT": "9", "SAGE_HIP_LUT2_SCALE": "256"}}


def bits(a):
    """an array as the words it is made of: equal means bit for bit (-0.0 is not 0.0, an entry is its peptide and its m/z)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a.view(np.uint32)


def same(got, want, what):
    got, want = bits(got).reshape(-1), bits(want).reshape(-1)
    assert len(got) == len(want), f"{what}: {len(got)} elements, the reference has {len(want)}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} elements differ, first at {i}: 0x{int(got[i]):x}, the reference has 0x{int(want[i]):x}")


def read_back(dev):
    return dev.layout(), {name: dev.table(name) for name in TABLES}


def create(monkeypatch, env, host, **kw):
    """environment variables are read at creation"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return DeviceDatabase(host, 0, **kw)


def expected_geometry(env):
    s1 = min(15, max(11, int(env.get("SAGE_HIP_TILE_SHIFT", 15))))
    s2 = min(16, max(6, int(env.get("SAGE_HIP_TILE2_SHIFT", 11))))
    return s1, 256.0, s2, float(env.get("SAGE_HIP_LUT2_SCALE", 32))


def reference_tables(ref, env):
    """the reference's position tables under `env`'s geometry (computed once, compared with both routes)"""
    s1, scale1, s2, scale2 = expected_geometry(env)
    lut2 = ref.position_table(s2, scale2)
    return ref.position_table(s1, scale1), lut2, succinct(lut2)


def compare_with_reference(ref, env, want, layout, t, route):
    """the layout and every table of one device database against the reference"""
    s1, scale1, s2, scale2 = expected_geometry(env)
    lut, lut2, (words, l1, pos) = want
    assert (layout["tile_shift"], layout["lut_scale"], layout["tile2_shift"], layout["lut2_scale"]) == (s1, scale1, s2, scale2), route
    assert (layout["np"], layout["nf"]) == (ref.np, ref.nf), route
    same(t["ions"], ref.ions, f"{route}: ions")
    same(t["ion_off"], ref.ion_off, f"{route}: ion_off")
    same(t["pm_off"], ref.pm_off, f"{route}: pm_off")
    same(t["pep_info"], ref.pep_info, f"{route}: pep_info")
    same(t["pep_mono"], ref.pep_mono, f"{route}: pep_mono")
    assert (layout["max_ions"], layout["max_len"]) == (ref.max_ions, ref.max_len), route
    assert (layout["ion_lo_bits"], layout["ion_hi_bits"]) == (ref.ion_lo_bits, ref.ion_hi_bits), f"{route}: |ion| range"
    # the large tiles
    same(t["tm_frag"], ref.tile_copy(s1), f"{route}: tm_frag")
    assert (layout["n_tiles"], layout["lut_stride"]) == lut.shape, f"{route}: n_tiles, lut_stride against {lut.shape}"
    same(t["tm_lut"], lut, f"{route}: tm_lut")
    # the small tiles and their table in succinct form
    same(t["tm2_frag"], ref.tile_copy(s2), f"{route}: tm2_frag")
    assert (layout["n_tiles2"], layout["lut2_stride"], layout["lut2_words"]) == lut2.shape + (words,), f"{route}: against {lut2.shape}, {words}"
    same(t["tm2_l1"]["bits"], l1["bits"], f"{route}: tm2_l1 occupancy bits")
    same(t["tm2_l1"]["rank"], l1["rank"], f"{route}: tm2_l1 ranks")
    assert layout["tm2_pos_len"] == len(t["tm2_pos"])
    same(t["tm2_pos"], pos, f"{route}: tm2_pos")
    same(decode(t["tm2_l1"], t["tm2_pos"], *lut2.shape), lut2, f"{route}: decode(tm2_l1, tm2_pos) against the row-major table")
    # the peptide-mass table
    bins, inv_w, pep_lut = ref.pep_lut()
    assert (layout["pep_lut_bins"], layout["pep_lut_inv_w"]) == (bins, float(inv_w)), f"{route}: peptide-mass table {bins} bins of 1/{inv_w}"
    same(t["pep_lut"], pep_lut, f"{route}: pep_lut")
    # the peptide-major list made again from the large-tile copy: per peptide in ascending total order of m/z, then the padding
    same(t["pm_frag"], ref.peptide_major_sorted(), f"{route}: pm_frag (rebuilt)")


def check_database(monkeypatch, env, ref, device_host, host_with_fragments, device_kw={}):
    """both routes against the reference and against each other; the generated peptide-major list of the device route"""
    dev = create(monkeypatch, env, device_host, **device_kw)
    layout_d, tables_d = read_back(dev)
    dev.close()
    want = reference_tables(ref, env)
    lut, lut2 = want[0], want[1]
    compare_with_reference(ref, env, want, layout_d, tables_d, "device route")
    dev = create(monkeypatch, dict(env, SAGE_HIP_KEEP_PM_FRAG="1"), device_host, **device_kw)
    same(dev.table("pm_frag"), ref.entries, "device route, SAGE_HIP_KEEP_PM_FRAG=1: pm_frag as generated (peptide, kind, ion index)")
    dev.close()
    dev = create(monkeypatch, env, host_with_fragments)
    layout_h, tables_h = read_back(dev)
    dev.close()
    compare_with_reference(ref, env, want, layout_h, tables_h, "host route")
    assert layout_d == layout_h, f"the two routes' layouts differ (both equal the reference's?): {layout_d} / {layout_h}"
    for name in TABLES:
        same(tables_d[name], tables_h[name], f"device route against host route: {name}")
    return layout_d, tables_d, lut, lut2


# ---- digest-built --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=ORDER)
def world(request, gpu_required):
    host = DatabaseParameters(**WORLDS[request.param][0]).build(synthetic_fasta(60, seed=31 + ORDER.index(request.param)))
    assert host.has_fragments
    return host, IndexReference(host)  # (one reference per world: its tile copies are shared by the geometries)


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_digest_built_index(world, geometry, monkeypatch):
    host, ref = world
    layout, t, lut, lut2 = check_database(monkeypatch, GEOMETRIES[geometry], ref, host, host, device_kw=dict(build_on_device=True))
    assert layout["n_tiles2"] > 1 and layout["nf"] > 10000


# ---- hand-built ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HAND_BUILT, ids=[c[0] for c in HAND_BUILT])
def test_hand_built_index(case, monkeypatch, gpu_required):
    name, env, build = case
    db = build()
    ref = IndexReference(db)
    # (the host route of a hand-built list: the stored entries by m/z, as Parameters::build would hand them over — the host then
    # computes the ion table, groups, sorts and tabulates on its own)
    layout, t, lut, lut2 = check_database(monkeypatch, env, ref, db, db.with_fragments(ref.sorted_entries()))
    mz2, toff2 = t["tm2_frag"]["fragment_mz"], ref.tile_offsets(layout["tile2_shift"])
    rows = t["tm_lut"].reshape(layout["n_tiles"], layout["lut_stride"])
    if name.startswith("seam_small") or name.startswith("seam_large"):
        n = int(name.rsplit("_", 1)[1])
        shift = layout["tile2_shift"] if "small" in name else layout["tile_shift"]
        assert (layout["n_tiles2"] if "small" in name else layout["n_tiles"]) == (n + (1 << shift) - 1) >> shift
    if name == "seam_large_4133":
        assert layout["nf"] > 200000  # (rocprim's multi-block sort and scan)
    if name == "tiny":
        assert layout["nf"] < 500     # (... and their single-block paths)
    if name == "empty_middle":
        w = t["tm2_l1"].reshape(layout["n_tiles2"], layout["lut2_words"])
        row = decode(t["tm2_l1"], t["tm2_pos"], layout["n_tiles2"], layout["lut2_stride"])[1]
        assert toff2[1] == toff2[2] and (row == toff2[1]).all(), "the empty tile's row: start == end in every cell"
        assert (w["bits"][1] == 0).all() and w["rank"][2, 0] - w["rank"][1, 0] == 1, "no bit set, one slot of tm2_pos (the tile's end)"
        assert t["tm2_pos"][w["rank"][1, 0]] == toff2[1]
    if name.startswith("signs"):
        for tile in range(layout["n_tiles2"]):
            m = mz2[toff2[tile]:toff2[tile + 1]]
            neg = int((m < 0).sum())
            assert (m[:neg] < 0).all() and (m[neg:] >= 0).all(), "negative m/z first within its tile"
            assert lut2[tile, 1] >= toff2[tile] + neg, "... and inside cell 0's run"
        top = mz2[:-2].max()
        assert layout["lut2_stride"] == int(np.ceil(float(top) * 32.0)) + 3 and top > 0, "the table's width: the largest positive m/z"
    if name.startswith("cell_edges"):
        m = t["tm_frag"]["fragment_mz"][:-2]
        for c in np.unique(np.floor(m.astype(np.float64) * 256.0).astype(np.int64)):  # cell c's run: exactly the entries of [c, c + 1) / 256
            assert rows[0, c + 1] - rows[0, c] == int(((m >= c / 256.0) & (m < (c + 1) / 256.0)).sum()) or c + 1 == layout["lut_stride"] - 1
    if name == "ties":
        e = t["tm2_frag"][:-2]
        eq = e["fragment_mz"][1:].view(np.uint32) == e["fragment_mz"][:-1].view(np.uint32)
        same_tile = e["peptide_index"][1:] >> 6 == e["peptide_index"][:-1] >> 6
        assert (eq & same_tile).sum() > 10 and (e["peptide_index"][1:][eq & same_tile] >= e["peptide_index"][:-1][eq & same_tile]).all()
        assert (e["peptide_index"] == 0).sum() == 4 and ((e["peptide_index"][1:] == 0) & (e["peptide_index"][:-1] == 0) & eq).sum() == 1
    if name == "empty":
        assert (layout["n_tiles"], layout["lut_stride"], layout["n_tiles2"], layout["lut2_stride"], layout["pep_lut_bins"]) == (1, 3, 1, 3, 0)
        assert len(t["pep_lut"]) == 0 and len(t["ions"]) == 0 and len(t["tm2_pos"]) == 1 and t["tm2_pos"][0] == 0
        assert (t["tm_lut"] == 0).all() and len(t["tm_frag"]) == 2 and len(t["pm_frag"]) == 2


def test_read_back_contract(monkeypatch, gpu_required):
    """sage_hip_debug_db_table's own edges: a table that does not exist, an unknown id, a buffer that is too small"""
    import ctypes as C

    from sage_amd import _lib as L
    db = HAND_BUILT[0][2]()
    dev = create(monkeypatch, {"SAGE_HIP_NO_PEP_LUT": "1"}, db)
    assert len(dev.table("pep_lut")) == 0 and dev.layout()["pep_lut_bins"] == 0
    lib, size = L.load(), C.c_uint64()
    assert lib.sage_hip_debug_db_table(dev._h, 99, None, 0, C.byref(size)) != 0
    buf = np.zeros(1, np.uint32)
    assert lib.sage_hip_debug_db_table(dev._h, L.DB_TABLES["pep_mono"][0], buf.ctypes.data_as(C.c_void_p), 4, C.byref(size)) != 0
    assert size.value == 4 * db.n_peptides and buf[0] == 0
    dev.close()
