"""Worlds for the protein-group tests, built through the public layers from an incidence matrix (protein -> blocks): every block
is a peptide of 7-12 residues that ends in K, every protein a concatenation of blocks, digested with missed_cleavages 0 — so a
block shared between proteins is a shared peptide and DatabaseParameters.build gives the database.  Also the hand cases, with
the values worked out on paper.  TEST INFRASTRUCTURE (no test in this file).
"""
from dataclasses import dataclass
from typing import Dict, List

import numpy as np

from protein_groups_reference import World
from sage_amd import _lib as L
from sage_amd.api import DatabaseParameters

ALPHABET = "ACDEFGHILMNQSTVWY"
RESIDUE_MASS = dict(A=71.04, C=103.01, D=115.03, E=129.04, F=147.07, G=57.02, H=137.06, I=113.08, L=113.08, M=131.04, N=114.04,
                    Q=128.06, S=87.03, T=101.05, V=99.07, W=186.08, Y=163.06, K=128.09)


def make_blocks(rng, n: int) -> List[str]:
    """n distinct blocks: 6-11 residues of ALPHABET and a closing K; heavier than the database's 500 Da floor by a margin"""
    seen, out = set(), []
    while len(out) < n:
        s = "".join(ALPHABET[int(c)] for c in rng.integers(0, len(ALPHABET), int(rng.integers(6, 12)))) + "K"
        if s in seen or sum(RESIDUE_MASS[c] for c in s) + 18.01 < 560.0:
            continue
        seen.add(s)
        out.append(s)
    return out


@dataclass
class BuiltWorld:
    host: object                 # IndexedDatabase (peptides only)
    world: World                 # what the restatement reads
    target_of_block: Dict[str, int]
    targets: np.ndarray          # peptide indices
    decoys: np.ndarray


def build_world(incidence: List[List[int]], blocks: List[str], names=None, generate_decoys=True) -> BuiltWorld:
    """incidence[p] = the block ids of protein p, in sequence order"""
    names = names or [f"P{p + 1:05d}" for p in range(len(incidence))]
    fasta = "".join(f">{names[p]}\n{''.join(blocks[b] for b in row)}\n" for p, row in enumerate(incidence))
    host = DatabaseParameters(enzyme=dict(missed_cleavages=0, cleave_at="KR", restrict="P"),
                              generate_decoys=generate_decoys).build(fasta, peptides_only=True)
    decoy = np.asarray(host.decoy, dtype=bool)
    proteins_of, target_of_block = [], {}
    for i in range(host.n_peptides):
        tagged = host.peptide_proteins(i).split(";")
        if decoy[i] and generate_decoys:
            assert all(t.startswith("rev_") for t in tagged)
            tagged = [t[4:] for t in tagged]
        proteins_of.append(tagged)
        if not decoy[i]:
            target_of_block[host.peptide_string(i)] = i
    used = {blocks[b] for row in incidence for b in row}
    assert set(target_of_block) == used, "the digest does not hold exactly the intended target peptides"
    owners = {}
    for p, row in enumerate(incidence):
        for b in row:
            owners.setdefault(blocks[b], set()).add(names[p])
    for s, i in target_of_block.items():  # ... each with exactly the intended proteins
        assert sorted(proteins_of[i]) == sorted(owners[s])
    return BuiltWorld(host, World(proteins_of, decoy, "rev_", generate_decoys), target_of_block, np.flatnonzero(~decoy), np.flatnonzero(decoy))


def random_incidence(rng, n_proteins: int, n_blocks: int, shared=0.3):
    """every block in one protein, a fraction `shared` of them in one to three more; every protein has a block"""
    rows = [[] for _ in range(n_proteins)]
    for b in range(n_blocks):
        owners = {int(rng.integers(n_proteins))} if b >= n_proteins else {b}
        if rng.random() < shared:
            owners |= {int(x) for x in rng.integers(0, n_proteins, int(rng.integers(1, 4)))}
        for p in sorted(owners):
            rows[p].append(b)
    return rows


def ring_incidence(rng, n_proteins: int, n_blocks: int, n_rings: int):
    """As random_incidence, but the last proteins form `n_rings` rings of 3-6 proteins in which every block is shared by two
    neighbours and no protein has a block of its own: each ring needs add_largest_to_cover picks."""
    sizes = [int(rng.integers(3, 7)) for _ in range(n_rings)]
    ring_proteins, ring_blocks = sum(sizes), sum(sizes)
    rows = random_incidence(rng, n_proteins - ring_proteins, n_blocks - ring_blocks, shared=0.12)
    p0, b0 = n_proteins - ring_proteins, n_blocks - ring_blocks
    for size in sizes:
        ring = [[] for _ in range(size)]
        for k in range(size):
            ring[k].append(b0 + k)
            ring[(k + 1) % size].append(b0 + k)
        rows += ring
        b0 += size
    assert len(rows) == n_proteins and b0 == n_blocks
    return rows


def feature_table(built: BuiltWorld, rng, n: int, decoy_frac=0.25):
    """n PSM records over the world's peptides (label -1 exactly for decoy peptides), shaped like search output"""
    from sage_amd.synthetic import synthetic_features
    f, *_ = synthetic_features(n, seed=int(rng.integers(1 << 30)), decoy_frac=decoy_frac)
    is_decoy = f["label"] == -1
    if len(built.decoys) == 0:
        is_decoy[:] = False
    f["peptide_idx"] = np.where(is_decoy, rng.choice(built.decoys, n) if len(built.decoys) else 0, rng.choice(built.targets, n))
    f["label"] = np.where(is_decoy, -1, 1)
    return f


def draw_peptide_q(f, rng):
    """one q per peptide: a third below the 1 % threshold, a third between it and 1, the rest exactly 1.0, a few exactly 0.01"""
    peps, inv = np.unique(f["peptide_idx"], return_inverse=True)
    u = rng.random(len(peps))
    q = np.where(u < 0.35, rng.uniform(0.0, 0.0099, len(peps)), np.where(u < 0.7, rng.uniform(0.0101, 0.99, len(peps)), 1.0))
    q[rng.random(len(peps)) < 0.02] = 0.01
    return q.astype(np.float32)[inv]


def bare_features(peptide_idx, label):
    f = np.zeros(len(peptide_idx), dtype=L.FEATURE_DTYPE)
    f["peptide_idx"], f["label"] = peptide_idx, label
    f["spec_index"] = np.arange(len(f))
    return f


# ---- the hand cases ---------------------------------------------------------------------------------------------------------------
# Blocks by ascending mass, so by ascending peptide index: a < b < c < d.
A, B, C, D = "AAAAAGSK", "LLLLLIVK", "HHHHHHHK", "WWWWWYFK"
HAND_BLOCKS = [A, B, C, D]
NAN = float("nan")

# name -> (proteins as block lists, features [(block, decoy?, peptide_q)], protein_grouping, expected [(string, count)],
#          expected (n_groups, n_meta_peptides) of the last pass).  The derivations are in test_protein_groups_cpu.py.
HAND_CASES = {
    "subsumed": ([[A, B, C], [B]], [(A, 0, 0.0), (B, 0, 0.0), (C, 0, 0.0)], True, [("P1", 1), ("P1", 1), ("P1", 1)], (2, 2)),
    "indistinguishable": ([[A, B], [A, B]], [(A, 0, 0.0), (B, 0, 0.0)], True, [("P1/P2", 1), ("P1/P2", 1)], (1, 1)),
    "triangle": ([[A, B], [B, C], [C, A]], [(A, 0, 0.0), (B, 0, 0.0), (C, 0, 0.0)], True, [("P3", 1), ("P2", 1), ("P2;P3", 2)], (3, 3)),
    "outside_p": ([[A, B]], [(A, 0, 0.0), (B, 0, 1.0)], True, [("P1", 1), ("P1", 1)], (1, 1)),
    "pass_one_stays": ([[A, B], [B, C]], [(A, 0, 0.0), (B, 0, 0.5), (C, 0, 0.5)], True, [("P1", 1), ("P1", 1), ("P2", 1)], (2, 3)),
    "grouping_off": ([[A, B], [B]], [(A, 0, 0.0), (B, 0, 0.0), (A, 1, 0.0)], False, [("P1", 1), ("P1;P2", 2), ("rev_P1", 1)], (0, 0)),
    "at_threshold": ([[A, B], [B], [C, D], [D]], [(A, 0, 0.01), (B, 0, 0.0), (C, 0, 1.0), (D, 0, 0.5)], True,
                     [("P1/P2", 1), ("P1/P2", 1), ("P3/P4", 1), ("P3/P4", 1)], (3, 3)),
    "nan_q": ([[A, B], [B]], [(A, 0, NAN), (B, 0, 0.0)], True, [("P1/P2", 1), ("P1/P2", 1)], (1, 1)),
    "no_targets": ([[A, B], [B]], [(A, 1, 0.0), (B, 1, 0.0)], True, [("rev_P1", 1), ("rev_P1;rev_P2", 2)], (0, 0)),
}


def hand_case(name):
    """-> (BuiltWorld, features, peptide_q, protein_grouping, expected rows, expected sizes)"""
    proteins, feats, grouping, expected, sizes = HAND_CASES[name]
    ids = {s: i for i, s in enumerate(HAND_BLOCKS)}
    built = build_world([[ids[s] for s in row] for row in proteins], HAND_BLOCKS, names=[f"P{p + 1}" for p in range(len(proteins))])
    decoy_of = {}
    for s, t in built.target_of_block.items():  # the decoy made from a target: its reversed interior, same proteins
        rev = s[0] + s[1:-1][::-1] + s[-1]
        hits = [int(i) for i in built.decoys if built.host.peptide_string(int(i)) == rev]
        if hits:
            decoy_of[s] = hits[0]
    idx = [decoy_of[s] if d else built.target_of_block[s] for s, d, _ in feats]
    f = bare_features(idx, [-1 if d else 1 for _, d, _ in feats])
    q = np.array([x for _, _, x in feats], dtype=np.float32)
    return built, f, q, grouping, expected, sizes
