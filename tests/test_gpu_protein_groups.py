"""sage_hip_protein_groups on the device against the plain-Python restatement (tests/protein_groups_reference.py): strings,
counts and graph sizes for equality; protein_group_q and the passing count against fdr.rs:42-120 read in numpy (picked_q_of) over
the restatement's keys and the same discriminants.  Both routes of the set cover (edge-parallel kernels, one workgroup with the
edges in LDS) and the hand-over between them are forced through SAGE_HIP_COVER_LDS_EDGES.
"""
import json
import os

import numpy as np
import pytest

import oracle_lib
import protein_groups_reference as ref
from protein_groups_worlds import (HAND_CASES, bare_features, build_world, draw_peptide_q, feature_table, hand_case, make_blocks,
                                   random_incidence, ring_incidence)
from rescore_edge_cases import picked_q_of
from sage_amd import cli, output
from sage_amd.api import DatabaseParameters, protein_groups
from sage_amd.synthetic import synthetic_fasta, synthetic_spectra
from sage_amd.mzml import write_mzml

pytestmark = pytest.mark.gpu

LDS_CAP_MAX = 18432  # include/sage_hip.h: the largest SAGE_HIP_COVER_LDS_EDGES


def kde_of_winners(winner, winner_decoy, queries):
    return oracle_lib.kde(winner, winner_decoy.astype(np.uint8), True, 1000, 1.0, queries, det=True)[3]


def expected_of(world, f, q, score, grouping=True, fdr=0.01):
    want = ref.generate_protein_groups(world, f["label"], f["peptide_idx"], q, grouping, fdr)
    keys, n_keys = ref.competition_keys(want["strings"], want["num"])
    decoy = np.array([world.decoy[int(p)] for p in f["peptide_idx"]], dtype=bool)
    want["q"] = picked_q_of(keys, n_keys, decoy, score, kde_of_winners)
    takes_part = (keys != ref.NO_KEY) & ~decoy
    want["passing"] = len(set(keys[takes_part & (want["q"] <= np.float32(0.01))].tolist()))
    return want


def assert_equal(got, want, context):
    assert [got.protein_groups(i) for i in range(len(got.string_id))] == want["strings"], context
    assert np.array_equal(got.num_protein_groups, want["num"]), context
    assert (got.n_groups, got.n_meta_peptides, got.cover_rounds) == (want["n_groups"], want["n_meta_peptides"], want["picks"]), context
    assert np.array_equal(got.protein_group_q, want["q"]), context
    assert got.passing_protein_group == want["passing"], context


def scores_for(f, rng):
    """discriminants shaped like the rescoring's: decoys low, targets mixed"""
    return np.where(f["label"] == -1, rng.normal(-1.0, 1.0, len(f)), rng.normal(1.5, 2.0, len(f))).astype(np.float32)


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_cases(name, gpu_required):
    """the cases of tests/test_protein_groups_cpu.py (derived on paper there), through the device"""
    built, f, q, grouping, expected, sizes = hand_case(name)
    score = np.linspace(3.0, -1.0, len(f)).astype(np.float32)
    got = protein_groups(built.host, f, q, score, grouping, 0.01)
    assert [(got.protein_groups(i), int(got.num_protein_groups[i])) for i in range(len(f))] == expected
    assert (got.n_groups, got.n_meta_peptides) == sizes
    assert_equal(got, expected_of(built.world, f, q, score, grouping), name)


def test_small_random_worlds(gpu_required):
    """30 worlds of about 40 proteins and 150 features, decoy features included, peptide_q drawn so that both passes select"""
    rng = np.random.default_rng(77)
    blocks = make_blocks(rng, 160)
    both = 0
    for w in range(30):
        n_proteins = int(rng.integers(30, 51))
        built = build_world(random_incidence(rng, n_proteins, int(rng.integers(n_proteins, 161)), shared=float(rng.uniform(0.2, 0.8))), blocks)
        f = feature_table(built, rng, 150)
        q, score = draw_peptide_q(f, rng), scores_for(f, rng)
        want = expected_of(built.world, f, q, score)
        both += want["selected"][0] > 0 and want["selected"][1] > want["selected"][0]
        assert (f["label"] == -1).any()
        assert_equal(protein_groups(built.host, f, q, score), want, w)
        if w % 10 == 0:  # ... and with grouping off, and with another threshold
            assert_equal(protein_groups(built.host, f, q, score, False), expected_of(built.world, f, q, score, False), (w, "off"))
            assert_equal(protein_groups(built.host, f, q, score, True, 0.5), expected_of(built.world, f, q, score, True, 0.5), (w, 0.5))
    assert both == 30


def test_without_the_pool_the_outputs_are_the_pooled_ones(gpu_required, monkeypatch):
    """the first world of test_small_random_worlds with SAGE_HIP_NO_POOL=1 (read once per call): every scratch buffer a plain
    hipMalloc, the outputs those of the pooled call and of the restatement"""
    rng = np.random.default_rng(77)
    blocks = make_blocks(rng, 160)
    n_proteins = int(rng.integers(30, 51))
    built = build_world(random_incidence(rng, n_proteins, int(rng.integers(n_proteins, 161)), shared=float(rng.uniform(0.2, 0.8))), blocks)
    f = feature_table(built, rng, 150)
    q, score = draw_peptide_q(f, rng), scores_for(f, rng)
    monkeypatch.delenv("SAGE_HIP_NO_POOL", raising=False)
    pooled = protein_groups(built.host, f, q, score)
    monkeypatch.setenv("SAGE_HIP_NO_POOL", "1")
    got = protein_groups(built.host, f, q, score)
    assert_equal(got, expected_of(built.world, f, q, score), "no pool")
    for name, x in vars(got).items():
        if name not in ("device_ms", "host_graph_ms"):  # (the two measured times)
            y = getattr(pooled, name)
            assert x == y if isinstance(x, (list, int)) else np.array_equal(x, y, equal_nan=True), name


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_large_worlds_on_both_routes(seed, gpu_required, monkeypatch):
    """3 000 proteins, 12 000 blocks, 20 000 features, rings that need add_largest_to_cover picks: the default cap, the bulk route
    alone (cap 0), the endgame from the first round (cap above the edge count) and a hand-over in between (a third of it) give
    the same outputs, equal to the restatement's"""
    rng = np.random.default_rng(1000 + seed)
    blocks = make_blocks(rng, 12000)
    built = build_world(ring_incidence(rng, 3000, 12000, 160), blocks)
    f = feature_table(built, rng, 20000)
    q, score = draw_peptide_q(f, rng), scores_for(f, rng)
    want = expected_of(built.world, f, q, score)
    assert want["picks"] >= 50, want["picks"]
    assert want["selected"][0] > 0 and want["selected"][1] > want["selected"][0]
    edges = max(want["edges"])
    assert 3000 < edges < LDS_CAP_MAX
    for cap in (None, 0, edges + 1, edges // 3):
        if cap is None:
            monkeypatch.delenv("SAGE_HIP_COVER_LDS_EDGES", raising=False)
        else:
            monkeypatch.setenv("SAGE_HIP_COVER_LDS_EDGES", str(cap))
        assert_equal(protein_groups(built.host, f, q, score), want, (seed, cap))


@pytest.mark.parametrize("n_edges", [63, 64, 65, 1023, 1025])
def test_edge_counts_at_the_wavefront_and_workgroup_seams(n_edges, gpu_required, monkeypatch):
    """a ring of n_edges // 2 proteins (two edges each, every pick a tie) and, for an odd count, one protein with a block of its
    own: exactly n_edges edges, on the endgame route, the bulk route and with a hand-over"""
    size = n_edges // 2
    rows = [[k, (k + size - 1) % size] for k in range(size)] + ([[size]] if n_edges % 2 else [])
    rng = np.random.default_rng(n_edges)
    built = build_world(rows, make_blocks(rng, size + 1))
    f = bare_features(built.targets, np.ones(len(built.targets), np.int32))
    q, score = np.zeros(len(f), np.float32), rng.normal(0, 1, len(f)).astype(np.float32)
    want = expected_of(built.world, f, q, score)
    assert want["edges"] == [n_edges, n_edges] and want["picks"] >= size // 2
    for cap in (None, 0, n_edges // 2):
        if cap is None:
            monkeypatch.delenv("SAGE_HIP_COVER_LDS_EDGES", raising=False)
        else:
            monkeypatch.setenv("SAGE_HIP_COVER_LDS_EDGES", str(cap))
        assert_equal(protein_groups(built.host, f, q, score), want, (n_edges, cap))


def test_empty_selection_and_one_feature(gpu_required):
    rng = np.random.default_rng(5)
    built = build_world(random_incidence(rng, 12, 40, shared=0.5), make_blocks(rng, 40))
    f = feature_table(built, rng, 60)
    score = scores_for(f, rng)
    q = np.ones(len(f), np.float32)  # 1.0 < 1.0 is false: no pass selects anything, every feature ends in the fallback
    want = expected_of(built.world, f, q, score)
    assert want["selected"] == [0, 0] and want["n_groups"] == 0
    assert_equal(protein_groups(built.host, f, q, score), want, "empty selection")
    for label in (1, -1):  # n = 1
        one = bare_features([int((built.targets if label == 1 else built.decoys)[3])], [label])
        for q1 in (0.0, 1.0):
            q, score = np.array([q1], np.float32), np.array([2.5], np.float32)
            assert_equal(protein_groups(built.host, one, q, score), expected_of(built.world, one, q, score), (label, q1))
    none = protein_groups(built.host, f[:0], q[:0], score[:0])  # n = 0
    assert none.strings == [] and none.passing_protein_group == 0 and len(none.protein_group_q) == 0


def test_cli_writes_the_group_columns(tmp_path, gpu_required):
    """a two-file synthetic search with `protein_grouping` in the configuration: the three columns of results.sage.tsv equal the
    restatement computed from the file's own peptide_q, label and sage_discriminant_score columns; the log and results.json carry
    the count.  Without the key the columns keep their defaults."""
    fasta = synthetic_fasta(80, seed=31)
    fa = str(tmp_path / "db.fasta")
    open(fa, "w").write(fasta)
    dbj = {"enzyme": {"missed_cleavages": 1, "cleave_at": "KR", "restrict": "P"}, "static_mods": {"C": 57.0215}, "fasta": fa}
    host = DatabaseParameters.from_json(dbj).build(fasta, peptides_only=True)
    files = []
    for k in range(2):
        p = str(tmp_path / f"run{k}.mzML")
        write_mzml(p, synthetic_spectra(DatabaseParameters.from_json(dbj).build(fasta), 300, seed=40 + k))
        files.append(p)
    cfg = {"database": dbj, "precursor_tol": {"ppm": [-10, 10]}, "fragment_tol": {"ppm": [-10, 10]}, "report_psms": 2,
           "mzml_paths": files, "protein_grouping": True}
    out = str(tmp_path / "o")
    logs = []
    summary = cli.run(cfg, files, out, log=logs.append)
    lines = open(os.path.join(out, "results.sage.tsv")).read().splitlines()
    hdr, rows = lines[0].split("\t"), [l.split("\t") for l in lines[1:]]
    assert hdr == output.HEADERS and len(rows) > 60
    col = lambda name: [r[hdr.index(name)] for r in rows]
    decoy = np.asarray(host.decoy, dtype=bool)
    index = {(host.peptide_string(i), bool(decoy[i])): i for i in range(host.n_peptides)}
    label = np.array([int(x) for x in col("label")])
    idx = [index[(s, l == -1)] for s, l in zip(col("peptide"), label)]
    proteins_of = [[t[4:] if decoy[i] else t for t in host.peptide_proteins(i).split(";")] for i in range(host.n_peptides)]
    world = ref.World(proteins_of, decoy, "rev_", True)
    f = bare_features(idx, label)
    q = np.array([np.float32(x) for x in col("peptide_q")], np.float32)
    score = np.array([np.float32(x) for x in col("sage_discriminant_score")], np.float32)
    want = expected_of(world, f, q, score)
    print("peptide_q < 0.01 / < 1.0 / rows:", int((q < 0.01).sum()), int((q < 1.0).sum()), len(q), "selected", want["selected"])
    assert col("protein_groups") == want["strings"] and [int(x) for x in col("num_protein_groups")] == want["num"].tolist()
    assert col("protein_group_q") == [output.ryu_f32(x) for x in want["q"]]
    assert summary["q_protein_group"] == want["passing"] and summary["protein_groups"] == want["n_groups"] > 0
    assert f"discovered {want['passing']} target protein groups (supported by proteotypic peptides only) at 1% FDR" in logs
    saved = json.load(open(os.path.join(out, "results.json")))
    assert saved["summary"]["q_protein_group"] == want["passing"]
    # the same search without the key: today's columns
    plain = str(tmp_path / "plain")
    summary = cli.run({k: v for k, v in cfg.items() if k != "protein_grouping"}, files, plain, log=lambda m: None)
    lines = open(os.path.join(plain, "results.sage.tsv")).read().splitlines()
    rows2 = [l.split("\t") for l in lines[1:]]
    assert "q_protein_group" not in summary and len(rows2) == len(rows)
    assert {(r[3], r[5], r[41]) for r in rows2} == {("", "0", "1.0")}
