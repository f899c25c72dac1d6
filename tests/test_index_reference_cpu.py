"""The numpy restatement of the fragment index (tests/index_reference.py) held to the oracle, to the host build and to the
emulation of core.h — before tests/test_gpu_index_tables.py holds the device's tables to it.  A comparison is only as good as
its reference: the stored entries must be the oracle's and the host's bit for bit, the ion table must reproduce them through the
keep rule, and the position tables must be the ones core.h's lut_entry / lut_rank define (tests/hostemu)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from index_cases import HAND_BUILT
from index_reference import IndexReference, decode, succinct, total_order_key
from sage_amd.api import DatabaseParameters
from sage_amd.synthetic import synthetic_fasta
from test_core_emulation import emu, fp  # noqa: F401  (the fixture that builds tests/hostemu)
from test_gpu_fuzz import ORDER, WORLDS


def by_mz_then_peptide(pep, mz):
    order = np.lexsort((pep, total_order_key(mz)))
    return pep[order], mz[order].view(np.uint32)


@pytest.fixture(scope="module", params=ORDER)
def world(request):
    params = DatabaseParameters(**WORLDS[request.param][0])
    fasta = synthetic_fasta(60, seed=31 + ORDER.index(request.param))
    host = params.build(fasta)
    return request.param, params, fasta, host, IndexReference(host)


def test_stored_entries_are_the_host_builds_and_the_oracles(world):
    name, params, fasta, host, ref = world
    assert ref.nf > 1000 and ref.nf == host.n_fragments, name
    mine = ref.sorted_entries()
    mp, mm = mine["peptide_index"], mine["fragment_mz"].view(np.uint32)
    assert np.isfinite(mine["fragment_mz"]).all()
    hp, hm = by_mz_then_peptide(host.fragments["peptide_index"], host.fragments["fragment_mz"])
    np.testing.assert_array_equal(mp, hp, err_msg=f"{name}: peptides of the stored entries, host build")
    np.testing.assert_array_equal(mm, hm, err_msg=f"{name}: m/z bits of the stored entries, host build")
    orc = oracle_lib.OracleDb.build(fasta, params).arrays()
    np.testing.assert_array_equal(orc["pep_mono"].view(np.uint32), host.pep_mono.view(np.uint32), err_msg=f"{name}: the two peptide lists")
    op, om = by_mz_then_peptide(orc["frag_pep"], orc["frag_mz"])
    np.testing.assert_array_equal(mp, op, err_msg=f"{name}: peptides of the stored entries, oracle")
    np.testing.assert_array_equal(mm, om, err_msg=f"{name}: m/z bits of the stored entries, oracle")


def test_ion_table_restricted_by_the_keep_rule_reproduces_the_entries(world):
    name, params, fasta, host, ref = world
    p, m = ref.restricted_ion_table()
    np.testing.assert_array_equal(p, ref.entries["peptide_index"], err_msg=name)
    np.testing.assert_array_equal(m.view(np.uint32), ref.entries["fragment_mz"].view(np.uint32), err_msg=name)
    hp, hm = by_mz_then_peptide(host.fragments["peptide_index"], host.fragments["fragment_mz"])
    rp, rm = by_mz_then_peptide(p, m)
    assert np.array_equal(rp, hp) and np.array_equal(rm, hm), name
    # every peptide's share of the table: (len - 1) ions per kind
    lens = np.diff(host.seq_off.astype(np.int64))
    np.testing.assert_array_equal(np.diff(ref.ion_off.astype(np.int64)), np.maximum(lens - 1, 0) * len(host.ion_kinds))
    np.testing.assert_array_equal(ref.pep_info & 0xFFFF, lens)
    np.testing.assert_array_equal((ref.pep_info >> 16) & 0xFF, host.decoy)
    np.testing.assert_array_equal(ref.pep_info >> 24, host.missed_cleavages)


@pytest.mark.parametrize("shift,scale", [(6, 8.0), (6, 32.0), (9, 256.0)])
def test_position_tables_are_core_h_tables(world, emu, shift, scale):
    """One tile in the middle of the index (a non-zero base) through core.h's lut_entry and its succinct form's check
    (emu_succinct_lut_mismatches: lut_rank against that row); every tile through the restatement's own decode."""
    name, params, fasta, host, ref = world
    emu.emu_lut_row.restype = None
    emu.emu_lut_row.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    copy = ref.tile_copy(shift)
    assert len(copy) == ref.nf + 2 and (copy[-2:]["peptide_index"] == 0xFFFFFFFF).all() and (copy[-2:]["fragment_mz"].view(np.uint32) == 0).all()
    toff = ref.tile_offsets(shift)
    first_tile = max(ref.n_tiles(shift) // 2 - 1, 0)
    lut = ref.position_table(shift, scale, range(first_tile, first_tile + 3))  # (three rows: the ranks cross two tile ends)
    toff = toff[first_tile:]
    n_tiles, stride = lut.shape
    assert ref.n_tiles(shift) >= 3 and stride == ref.stride(scale) and len(toff) >= 4
    t = 1
    mz = np.ascontiguousarray(copy["fragment_mz"][toff[t]:toff[t + 1]])
    assert len(mz) > 0 and (np.diff(total_order_key(mz)) >= 0).all()
    row = np.zeros(stride, np.uint32)
    emu.emu_lut_row(fp(mz), len(mz), scale, stride, int(toff[t]), row.ctypes.data_as(C.POINTER(C.c_uint32)))
    np.testing.assert_array_equal(lut[t], row, err_msg=f"{name}: row of tile {t}")
    words, l1, pos = succinct(lut)
    nonempty = C.c_uint64()
    assert emu.emu_succinct_lut_mismatches(fp(mz), len(mz), scale, stride, 12345, C.byref(nonempty)) == 0
    w = l1.reshape(n_tiles, words)
    first, last = int(w["rank"][t, 0]), int(w["rank"][t + 1, 0]) if t + 1 < n_tiles else len(pos)
    assert last - first == nonempty.value + 1, "run starts of the tile's non-empty cells, then the tile's end"
    assert pos[last - 1] == toff[t + 1] and len(pos) == int((lut[:, 1:] != lut[:, :-1]).sum()) + n_tiles
    np.testing.assert_array_equal(decode(l1, pos, n_tiles, stride), lut, err_msg=f"{name}: decode(succinct(table))")
    # the table is what a plain count says: entries of the tile below the cell's edge
    for c in (1, stride // 3, stride - 2):
        assert lut[t, c] == toff[t] + int((mz.astype(np.float64) < c / scale).sum())


@pytest.mark.parametrize("case", HAND_BUILT, ids=[c[0] for c in HAND_BUILT])
def test_hand_built_databases_stay_inside_the_contract(case):
    """What the GPU tests feed the device: finite m/z only (NaN and infinities are outside the contract: the host's scan and the
    device's binary search are not defined to agree on them), an ascending peptide list, and the property each case is there for."""
    name, env, build = case
    db = build()
    ref = IndexReference(db)
    assert np.isfinite(ref.ions).all() and np.isfinite(ref.entries["fragment_mz"]).all()
    assert (np.diff(total_order_key(db.pep_mono)) >= 0).all()
    mz, pep = ref.entries["fragment_mz"], ref.entries["peptide_index"]
    if name == "seam_large_4133":
        assert ref.nf > 200000
    if name == "tiny":
        assert 0 < ref.nf < 500
    if name == "empty":
        assert ref.np == 0 and ref.nf == 0 and ref.pep_lut()[0] == 0 and ref.stride(32.0) == 3
    if name == "empty_middle":
        assert ref.pm_off[64] == ref.pm_off[128] and 0 < ref.pm_off[64] < ref.nf
    if name.startswith("signs"):
        assert (mz < 0).sum() >= 20 and (mz.view(np.uint32) == 0).sum() >= 8
    if name.startswith("lengths"):
        assert ref.max_len == 1500 and sorted(set(np.diff(db.seq_off.astype(np.int64)))) == [0, 1, 2, 3, 4, 40, 1500]
    if name.startswith("cell_edges"):
        on32 = mz * np.float32(32.0)
        on256 = mz * np.float32(256.0)
        assert (on32 == np.floor(on32)).sum() >= 4 and (on256 == np.floor(on256)).sum() >= 8
        top = mz.max()
        assert ref.stride(256.0) == int(np.ceil(float(top) * 256.0)) + 3
        if name in ("cell_edges_top_k32", "cell_edges_top_k256"):  # the largest m/z opens the table's last real cell
            assert float(top) * 256.0 == ref.stride(256.0) - 3
    if name == "ties":
        first = ref.entries[pep == 0]["fragment_mz"]
        assert len(first) == 4 and len(set(first.view(np.uint32))) == 3, "b1 == y1 for the first peptide"
        s = ref.sorted_entries()
        same = s["fragment_mz"][1:].view(np.uint32) == s["fragment_mz"][:-1].view(np.uint32)
        assert (same & (s["peptide_index"][1:] >> 6 != s["peptide_index"][:-1] >> 6)).any(), "equal m/z on both sides of a seam"
        assert (same & (s["peptide_index"][1:] >> 6 == s["peptide_index"][:-1] >> 6)).sum() > 10
    lut2 = ref.position_table(6, 32.0)
    words, l1, pos = succinct(lut2)
    assert np.array_equal(decode(l1, pos, *lut2.shape), lut2), name
