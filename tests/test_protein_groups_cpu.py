"""Protein groups without a GPU: the restatement (tests/protein_groups_reference.py) on hand cases worked out on paper, the host
graph builder (sage_hip_group_graph_build) and the shared round logic of the set cover (sage_amd/csrc/cover.h through
tests/hostemu/cover_emu.cpp) against the restatement on random worlds, and the grouped native writer against the Python row.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import protein_groups_reference as ref
from protein_groups_worlds import HAND_CASES, build_world, hand_case, make_blocks, random_incidence
from sage_amd import _lib as L
from sage_amd import cli, output

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "cover_emu.cpp")
LIB = os.path.join(HERE, "hostemu", "libcover_emu.so")
HEADER = os.path.join(HERE, "..", "sage_amd", "csrc", "cover.h")


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HEADER)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.emu_cover.restype = C.c_int
    lib.emu_cover.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                              C.POINTER(C.c_uint8)]
    return lib


@pytest.fixture(scope="module")
def random_worlds():
    """200 worlds of 5-60 proteins and 10-200 blocks with random incidence, each with a random selection of its targets and the
    restatement's graph of that selection; computed once, read by the tests below"""
    rng = np.random.default_rng(20240611)
    blocks = make_blocks(rng, 200)
    out = []
    for _ in range(200):
        n_proteins = int(rng.integers(5, 61))
        n_blocks = int(rng.integers(max(10, n_proteins), 201))
        built = build_world(random_incidence(rng, n_proteins, n_blocks, shared=float(rng.uniform(0.1, 0.8))), blocks)
        selected = np.sort(rng.choice(built.targets, int(rng.integers(1, len(built.targets) + 1)), replace=False))
        out.append((built, selected, ref.build_graph(built.world, selected.tolist())))
    return out


def emu_cover(emu, edges, n_left, n_right, reverse):
    el = np.ascontiguousarray([e[0] for e in edges], dtype=np.uint32)
    er = np.ascontiguousarray([e[1] for e in edges], dtype=np.uint32)
    cover = np.zeros(max(n_left, 1), np.uint8)
    picks = emu.emu_cover(L.as_ptr(el, C.c_uint32), L.as_ptr(er, C.c_uint32), len(edges), n_left, n_right, int(reverse),
                          L.as_ptr(cover, C.c_uint8))
    return [bool(x) for x in cover[:n_left]], picks


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_restatement_on_the_hand_cases(name):
    """Blocks a < b < c < d by mass, so by peptide index; P1, P2, ... in FASTA order; every feature is a target with the q given
    unless said otherwise; thresholds 0.01 then 1.0.

    subsumed           P1{a,b,c} P2{b}, all q 0.  Meta-peptides {P1} (a, c) and {P1,P2} (b).  {P1} has degree 1: P1 enters the
                       cover, its edges go and cover both meta-peptides, P2's edge goes with the covered {P1,P2}.  b: P1 only.
    indistinguishable  P1{a,b} P2{a,b}.  One meta-peptide {P1,P2}, both proteins have the evidence [0]: one group, P1/P2.
    triangle           P1{a,b} P2{b,c} P3{c,a}.  a is the lowest peptide, so P1 = 0, P3 = 1 (a's proteins), P2 = 2; meta-peptides
                       (0,1) (0,2) (1,2) = a, b, c; evidence P1 [0,1], P3 [0,2], P2 [1,2] = groups 0, 1, 2.  No right node of
                       degree 1.  All keys are (2, 2): the tie goes to group 2 = P2; its edges go, b and c are covered, the edges
                       P1-b and P3-c go.  Left: P1-a, P3-a, keys (1,2), (1,2), (0,2): the tie goes to group 1 = P3.  Cover
                       {P2, P3}: a (P1, P3) is P3, b (P1, P2) is P2, c (P2, P3) is P2;P3.
    outside_p          P1{a,b}, q(a) = 0, q(b) = 1.0: b is never selected (1.0 < 1.0 is false) but its protein P1 is in the
                       cover of pass 1, so b is annotated P1 there.
    pass_one_stays     P1{a,b} P2{b,c}, q = 0, 0.5, 0.5.  Pass 1 knows a only: cover {P1}, a and b (through P1) become P1, c has
                       no known protein.  Pass 2 knows all three, both proteins are forced, b would be P1;P2 — it keeps P1; c: P2.
    grouping_off       only the fallback: the stored protein list and its length; the decoy of a carries the tag.
    at_threshold       P1{a,b} P2{b} P3{c,d} P4{d}, q = 0.01, 0, 1.0, 0.5.  0.01 < 0.01 is false: pass 1 knows b only, P1 and P2
                       share the evidence, a (through P1) and b are P1/P2 (with a selected they would be P1).  Pass 2 selects d
                       and not c: P3/P4 for both (with c selected: P3).  Last pass: meta-peptides a, b, d; groups P1, P2, P3/P4.
    nan_q              P1{a,b} P2{b}, q(a) NaN: a is selected in no pass, b alone makes P1/P2 for both.
    no_targets         decoy features only: nothing is ever selected, no graph; the tagged fallback lists."""
    built, f, q, grouping, expected, sizes = hand_case(name)
    got = ref.generate_protein_groups(built.world, f["label"], f["peptide_idx"], q, grouping, 0.01)
    assert list(zip(got["strings"], got["num"].tolist())) == expected
    assert (got["n_groups"], got["n_meta_peptides"]) == sizes


def test_restatement_cover_on_the_reference_unit_cases():
    """the BipartiteGraph unit tests of protein_grouping.rs:477-515 and its ten-peptide example (:395-475)"""
    assert ref.into_cover([(0, 0), (1, 1), (2, 2)], 3, 3)[0] == [True, True, True]
    assert ref.into_cover([(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)], 2, 3)[0] == [True, False]
    assert ref.into_cover([(0, 0), (0, 1), (1, 1), (1, 2)], 2, 3)[0] == [True, True]
    assert ref.into_cover([], 0, 0) == ([], 0) and ref.into_cover([(0, 0)], 1, 1)[0] == [True]
    prots = [[7], [4, 6, 9], [1], [1, 5], [7], [3, 6], [1], [1, 2, 5, 8], [1], [4, 9]]
    world = ref.World([[f"protein_{p}" for p in row] for row in prots], [False] * 10, "rev_", False)
    got = ref.generate_protein_groups(world, [1] * 10, range(10), [0.0] * 10, True, 0.01)
    assert got["strings"] == ["protein_7", "protein_4/protein_9;protein_6", "protein_1", "protein_1", "protein_7", "protein_6",
                              "protein_1", "protein_1", "protein_1", "protein_4/protein_9"]


def test_host_graph_builder_matches_the_restatement(random_worlds):
    for built, selected, want in random_worlds:
        g = built.host.group_graph(selected)
        names = [(built.host.protein_name(int(i)), bool(d)) for i, d in zip(g.protein_id, g.protein_decoy)]
        assert names == want["proteins"]
        assert g.n_meta_peptides == len(want["metas"]) and g.n_groups == len(want["groups"])
        groups = [tuple(int(x) for x in g.group_proteins[int(g.group_off[k]):int(g.group_off[k + 1])]) for k in range(g.n_groups)]
        evidence = [tuple(int(x) for x in g.evidence[int(g.evidence_off[k]):int(g.evidence_off[k + 1])]) for k in range(g.n_groups)]
        assert groups == want["groups"] and evidence == want["evidence"]
        assert list(zip(g.edge_group.tolist(), g.edge_meta.tolist())) == want["edges"]
    empty = random_worlds[0][0].host.group_graph(np.zeros(0, np.uint32))
    assert empty.n_groups == 0 and empty.n_meta_peptides == 0 and len(empty.edge_group) == 0
    with pytest.raises(L.SageHipError):  # not ascending
        random_worlds[0][0].host.group_graph(np.array([3, 1], np.uint32))


def test_shared_round_logic_matches_the_sequential_cover(emu, random_worlds):
    """cover.h's three trim steps and argmax key, every step over all live edges at once (the device's schedule) and in both edge
    orders, against the sequential into_cover on the graphs of the same worlds"""
    some_picks = 0
    for _, _, graph in random_worlds:
        want, want_picks = ref.into_cover(graph["edges"], len(graph["groups"]), len(graph["metas"]))
        for reverse in (False, True):
            got, picks = emu_cover(emu, graph["edges"], len(graph["groups"]), len(graph["metas"]), reverse)
            assert got == want and picks == want_picks
        some_picks += want_picks
    assert some_picks > 0  # (some world needed add_largest_to_cover)
    for size in range(3, 12):  # rings: no unique evidence, every pick a tie
        edges = [(k, k) for k in range(size)] + [((k + 1) % size, k) for k in range(size)]
        want, want_picks = ref.into_cover(edges, size, size)
        assert emu_cover(emu, edges, size, size, False) == (want, want_picks) and want_picks >= 1


def test_round_logic_stand_alone_under_sanitizers(tmp_path):
    """the same emulation as a program of its own, with AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "cover_emu_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DCOVER_EMU_MAIN", SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cover_emu ok" in r.stdout, r.stdout + r.stderr


def test_grouped_native_writer_matches_the_python_rows(tmp_path):
    """sage_hip_write_results_grouped against output.feature_row with the three group columns, byte for byte; without the
    columns it writes what sage_hip_write_results writes"""
    from types import SimpleNamespace

    from sage_amd.synthetic import synthetic_features
    built = hand_case("triangle")[0]
    host = built.host
    n = 300
    f, *_ = synthetic_features(n, seed=5)
    rng = np.random.default_rng(6)
    f["peptide_idx"] = rng.integers(0, host.n_peptides, n)
    f["file_id"] = rng.integers(0, 2, n)
    strings = ["P1", "P2;P3", "rev_P1/rev_P2", 'odd "name"\twith a tab', ""]
    groups = SimpleNamespace(strings=strings, string_id=rng.integers(0, len(strings), n).astype(np.uint32),
                             num_protein_groups=rng.integers(0, 5, n).astype(np.uint32),
                             protein_group_q=rng.choice(np.array([1.0, 0.0, 0.25, 1e-7, 0.0123456], np.float32), n))
    post = SimpleNamespace(discriminant_score=rng.normal(0, 3, n).astype(np.float32), peptide_q=rng.uniform(0, 1, n).astype(np.float32))
    spec_ids = [f"scan={i}" for i in range(n)]
    psm_ids = np.arange(1, n + 1)
    order = rng.permutation(n)
    filenames = ["a.mzML", "b.mzML"]
    p = str(tmp_path / "grouped.tsv")
    output.write_results_native(p, "tsv", host, f, order, psm_ids, filenames, spec_ids, post, groups)
    want = ["\t".join(output.HEADERS)]
    for i in order:
        row = output.feature_row(int(psm_ids[i]), f[i], host, filenames[int(f["file_id"][i])], spec_ids[i],
                                 dict(discriminant_score=post.discriminant_score[i], peptide_q=post.peptide_q[i]),
                                 protein_groups=strings[int(groups.string_id[i])], num_protein_groups=int(groups.num_protein_groups[i]),
                                 protein_group_q=groups.protein_group_q[i])
        want.append("\t".join(output.csv_field(x) for x in row))
    got = open(p).read().split("\n")
    assert got[-1] == "" and got[:-1] == want, next((a, b) for a, b in zip(got, want) if a != b)
    q = str(tmp_path / "plain.tsv")
    output.write_results_native(q, "tsv", host, f, order, psm_ids, filenames, spec_ids, post)
    r = str(tmp_path / "refused.tsv")
    plain = open(q, "rb").read()
    assert plain != open(p, "rb").read()
    with pytest.raises(L.SageHipError, match="string id out of range"):
        output.write_results_native(r, "tsv", host, f, order, psm_ids, filenames, spec_ids, post,
                                    SimpleNamespace(strings=["x"], string_id=np.full(n, 7, np.uint32),
                                                    num_protein_groups=np.zeros(n, np.uint32), protein_group_q=np.ones(n, np.float32)))
    # the pin format has no group column: both entry points write the same file
    a, b = str(tmp_path / "a.pin"), str(tmp_path / "b.pin")
    output.write_results_native(a, "pin", host, f, order, psm_ids, filenames, spec_ids, post)
    output.write_results_native(b, "pin", host, f, order, psm_ids, filenames, spec_ids, post, groups)
    assert open(a, "rb").read() == open(b, "rb").read()
    # the default row of feature_row is today's row
    row = dict(zip(output.HEADERS, output.feature_row(1, f[0], host, "a.mzML", "s")))
    assert (row["protein_groups"], row["num_protein_groups"], row["protein_group_q"]) == ("", "0", "1.0")


def test_search_parameters_read_the_grouping_keys():
    """input.rs:382-383: protein_grouping absent -> true, protein_grouping_peptide_fdr absent -> 0.01; the stage runs in the CLI
    when the configuration names one of them"""
    base = {"precursor_tol": {"ppm": [-10, 10]}, "fragment_tol": {"ppm": [-10, 10]}}
    sp = cli.search_parameters(base)
    assert sp["protein_grouping"] is True and sp["protein_grouping_peptide_fdr"] == 0.01 and not sp["protein_group_stage"]
    sp = cli.search_parameters(dict(base, protein_grouping=False))
    assert sp["protein_grouping"] is False and sp["protein_group_stage"]
    sp = cli.search_parameters(dict(base, protein_grouping_peptide_fdr=0.05))
    assert sp["protein_grouping"] is True and sp["protein_grouping_peptide_fdr"] == 0.05 and sp["protein_group_stage"]


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(HERE, "..", "include", "sage_hip.h")).read()
    for name in ("sage_hip_protein_groups", "sage_hip_group_string", "sage_hip_group_strings_free", "sage_hip_group_graph_build",
                 "sage_hip_write_results_grouped"):
        assert f"{name}(" in hdr and name in L.EXPORTED_SYMBOLS and hasattr(L.load(), name)
    assert L.load().sage_hip_abi_version() == 6
    assert C.sizeof(L.SageGroupInput) == 40 and C.sizeof(L.SageGroupColumns) == 40
