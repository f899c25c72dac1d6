"""Positional-isomer groups of a host database (sage_hip_hostdb_isomer_groups) against the plain restatement
of the definition (tests/isomers_reference.py), array for array.  CPU only.  (The input validation of
sage_hip_score_candidates_resident needs a scorer and a resident batch, that is a device: tests/test_gpu_isomers.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import isomers_reference as IR
from sage_amd import _lib as L
from sage_amd.api import DatabaseParameters
from sage_amd.synthetic import synthetic_fasta


def _assert_groups_equal(host, context):
    got, want = host.isomer_groups(), IR.isomer_groups(host)
    for name, g, w in zip(("group_of", "group_off", "members"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{context}: {name} differs from the restatement"
    return got


def test_the_sixty_protein_phospho_world():
    host = DatabaseParameters(**IR.PHOSPHO_DB).build(synthetic_fasta(60, 7))
    group_of, group_off, members = _assert_groups_equal(host, "phospho world")
    # the figures the feature was planned on: a drift of the fixture should be noticed
    assert host.n_peptides == 73708
    assert int((group_of != IR.NONE).sum()) == 59498 == len(members)
    sizes = np.diff(group_off.astype(np.int64))
    assert sizes.min() >= 2 and sizes.max() == 120
    # why a neighbour scan over the masses cannot find the groups: members lie far apart and their f32 masses differ
    first, last = members[group_off[:-1].astype(np.int64)], members[group_off[1:].astype(np.int64) - 1]
    assert int((last.astype(np.int64) - first).max()) > 64
    spread = np.array([np.ptp(host.pep_mono[members[int(a):int(b)]]) for a, b in zip(group_off[:-1], group_off[1:])])
    assert spread.max() > 0
    # groups by ascending smallest member, members ascending
    assert np.all(np.diff(first.astype(np.int64)) > 0)
    for a, b in zip(group_off[:-1], group_off[1:]):
        assert np.all(np.diff(members[int(a):int(b)].astype(np.int64)) > 0)


def test_static_mods_only_give_no_group():
    host = DatabaseParameters(enzyme=IR.ENZYME, static_mods={"C": 57.0215, "K": 229.1629}).build(synthetic_fasta(60, 7))
    group_of, group_off, members = _assert_groups_equal(host, "static mods")
    assert host.n_peptides > 1000 and np.count_nonzero(host.mods) > 0
    assert len(group_off) == 1 and len(members) == 0 and np.all(group_of == IR.NONE)


@pytest.mark.parametrize("name,dbkw", [
    # a terminal modification and a residue modification of one mass share a group: acetyl on the peptide N-terminus or on K,
    # methyl on the peptide C-terminus or on E
    ("peptide_termini", dict(enzyme=IR.ENZYME, static_mods={"C": 57.0215},
                             variable_mods={"[": [42.010565], "K": [42.010565], "]": [14.01565], "E": [14.01565]}, max_variable_mods=2)),
    ("no_decoys", dict(IR.PHOSPHO_DB, generate_decoys=False)),
    ("three_variable_mods", dict(IR.PHOSPHO_DB, max_variable_mods=3, enzyme=dict(IR.ENZYME, missed_cleavages=0, max_len=25))),
    ("peptides_only", dict(IR.PHOSPHO_DB, peptides_only=True)),
])
def test_groups_equal_the_restatement(name, dbkw):
    host = DatabaseParameters(**dbkw).build(synthetic_fasta(40, 21))
    group_of, group_off, members = _assert_groups_equal(host, name)
    assert len(group_off) > 100, f"{name}: only {len(group_off) - 1} groups"
    if name == "peptide_termini":
        nterm = np.nan_to_num(host.nterm) != 0
        cterm = np.nan_to_num(host.cterm) != 0
        assert np.any(nterm & (group_of != IR.NONE)) and np.any(cterm & (group_of != IR.NONE))
        # some group holds a terminal placement next to a residue placement of the same mass
        mixed = 0
        for a, b in zip(group_off[:-1], group_off[1:]):
            m = members[int(a):int(b)]
            mixed += bool(nterm[m].any() and not nterm[m].all())
        assert mixed > 0
    if name == "no_decoys":
        assert not host.decoy.any()
    if name == "peptides_only":
        assert not host.has_fragments
        full = DatabaseParameters(**dict(dbkw, peptides_only=False)).build(synthetic_fasta(40, 21))
        for g, w in zip((group_of, group_off, members), full.isomer_groups()):
            assert np.array_equal(g, w)


def test_prefilter_merged_database():
    fasta = synthetic_fasta(40, 21)
    dbp = DatabaseParameters(**IR.PHOSPHO_DB)
    rng = np.random.default_rng(5)
    chunks, keeps = [], []
    for first in range(0, dbp.num_targets(fasta), 16):
        c = dbp.build_chunk(fasta, first, 16, peptides_only=True)
        chunks.append(c)
        keeps.append((rng.random(c.n_peptides) < 0.6).astype(np.uint8))
    host = dbp.merge_kept(chunks, keeps, peptides_only=True)
    assert 0 < host.n_peptides < sum(c.n_peptides for c in chunks)
    _, group_off, _ = _assert_groups_equal(host, "merge_kept")
    assert len(group_off) > 100


def test_sizing_call_and_null_handle():
    host = DatabaseParameters(**IR.PHOSPHO_DB).build(synthetic_fasta(40, 21))
    lib = L.load()
    ng, nm = C.c_uint64(), C.c_uint64()
    L.check(lib.sage_hip_hostdb_isomer_groups(host._h, None, None, None, C.byref(ng), C.byref(nm)))
    _, group_off, members = host.isomer_groups()
    assert (ng.value, nm.value) == (len(group_off) - 1, len(members))
    assert lib.sage_hip_hostdb_isomer_groups(None, None, None, None, C.byref(ng), C.byref(nm)) == 1  # SAGE_HIP_ERR_INVALID
    assert lib.sage_hip_hostdb_isomer_groups(host._h, None, None, None, None, None) == 1


def test_abi_version_and_exported_symbols():
    lib = L.load()
    assert lib.sage_hip_abi_version() == 6
    new = ["sage_hip_hostdb_isomer_groups", "sage_hip_score_candidates_resident", "sage_hip_last_candidates_timing"]
    assert all(s in L.EXPORTED_SYMBOLS for s in new)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sage_hip.h")).read()
    for s in new:
        assert f" T {s}\n" in dynamic, f"{s} is not exported"
        assert f" {s}(" in header, f"{s} is not declared in sage_hip.h"
    assert C.sizeof(C.c_double) + 3 * 4 + 5 * 4 == L.CANDIDATE_SCORE_DTYPE.itemsize == 40
