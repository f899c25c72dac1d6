"""Hand-built peptide lists for the index-table tests (test_index_reference_cpu.py, test_gpu_index_tables.py): the edges of
index_build.hip's kernels that a digest of a synthetic proteome reaches only by luck.  Every case is (id, environment at
DeviceDatabase creation, builder of an index_reference.ArrayDb); the lists are small and seeded.

pep_mono is an INPUT of the index (the host's digest delivers it, ascending): the cases compute it from the residues in f32 and
sort by it, or set it by hand where an exact coincidence is wanted (`mono=`)."""
import numpy as np

from index_reference import (ArrayDb, F32, KIND_A, KIND_B, KIND_C, KIND_X, KIND_Y, KIND_Z, RESIDUE_MASS, total_order_key)

AA = b"ACDEFGHIKLMNPQRSTVWY"
ODD = AA + b"UOBJXZ" + b"a7"  # selenocysteine, pyrrolysine, the four letters of mass 0, a lowercase byte and a digit (mass 0)
BY = (KIND_B, KIND_Y)
ALL = (KIND_A, KIND_B, KIND_C, KIND_X, KIND_Y, KIND_Z)
H2O = F32(18.010565)
G = RESIDUE_MASS[ord("G")]


class Pep:
    def __init__(self, seq, mods=None, nterm=np.nan, mono=None, decoy=0, missed=0):
        self.seq = bytes(seq)
        self.mods = np.zeros(len(self.seq), F32) if mods is None else np.asarray(mods, F32)
        assert len(self.mods) == len(self.seq)
        self.nterm = F32(nterm)
        self.decoy, self.missed = decoy, missed
        if mono is None:  # (any f32 sum will do: the index only needs the list ascending)
            mono = H2O + (F32(0.0) if np.isnan(self.nterm) else self.nterm)
            for r, m in zip(self.seq, self.mods):
                mono = F32(mono + F32(RESIDUE_MASS[r] + m))
        self.mono = F32(mono)


def database(peps, kinds=BY, min_ion_index=2, sort=True):
    if sort:  # ascending pep_mono (total order), ties in the given order
        order = np.argsort(total_order_key(np.array([p.mono for p in peps], F32)), kind="stable") if peps else []
        peps = [peps[i] for i in order]
    return ArrayDb([p.seq for p in peps], [p.mods for p in peps], [p.nterm for p in peps], [p.mono for p in peps], kinds, min_ion_index,
                   [p.decoy for p in peps], [p.missed for p in peps])


def random_peptides(rng, n, lo=3, hi=12, alphabet=AA, weights=None, modded=0.0):
    letters = np.frombuffer(alphabet, np.uint8)
    lens = rng.choice(np.arange(lo, hi + 1), size=n, p=weights)
    out = []
    for k in lens:
        seq = letters[rng.integers(0, len(letters), int(k))].tobytes()
        mods = np.where(rng.random(int(k)) < modded, rng.choice([15.9949, 79.9663, -17.0265, -18.0106, 57.0215], int(k)), 0.0)
        out.append(Pep(seq, mods, decoy=int(rng.random() < 0.5), missed=int(rng.integers(0, 3))))
    return out


def step_mod(residue, target):
    """an f32 modification mass m with f32(monoisotopic(residue) + m) == target exactly"""
    r, target = RESIDUE_MASS[residue], F32(target)
    m = F32(target - r)
    for _ in range(64):
        d = F32(r + m)
        if d == target:
            return m
        m = np.nextafter(m, F32(np.inf) if d < target else F32(-np.inf))
    raise AssertionError((residue, target))


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def seam_small(n):
    return lambda: database(random_peptides(np.random.default_rng([6, n]), n, modded=0.1))


def seam_large(n):
    if n == 4133:  # ... and more than 200 000 stored entries: six kinds, every ion stored, mostly long peptides
        w = np.array([0.04] * 7 + [0.24] * 3)
        return lambda: database(random_peptides(np.random.default_rng([11, n]), n, weights=w / w.sum()), ALL, 0)
    return lambda: database(random_peptides(np.random.default_rng([11, n]), n))


def empty_middle():
    """peptides 64..127 (a whole small tile at shift 6) have no stored entry: length <= min_ion_index + 1"""
    rng = np.random.default_rng(64)
    light = random_peptides(rng, 64, 4, 5, b"GAS")                     # <= 453 Da
    short = [Pep(p.seq, [500.0] + [0.0] * (len(p.seq) - 1)) for p in random_peptides(rng, 64, 1, 3, b"GAS")]  # 575 .. 780 Da
    heavy = random_peptides(rng, 64, 8, 12, b"WYFR")                   # >= 1176 Da
    db = database(light + short + heavy)
    lens = np.diff(db.seq_off.astype(np.int64))
    assert (lens[64:128] <= 3).all() and (lens[:64] >= 4).all() and (lens[128:] >= 8).all()
    return db


def lengths(kinds, min_ion_index):
    """0, 1, 2, 3, 4 and 40 residues — around every branch of the keep rule — beside one peptide of 1 500 (kept light by negative
    modifications: the table's width follows the largest m/z)"""
    def build():
        rng = np.random.default_rng(15)
        peps = [p for k in (0, 1, 2, 3, 4, 40) for p in random_peptides(rng, 2, k, k)]
        peps.append(Pep(b"G" * 1500, np.full(1500, -40.0, F32)))
        return database(peps, kinds, min_ion_index)
    return build


def termini(min_ion_index):
    """every N-terminal form x every kind x odd residues, modifications of both signs"""
    def build():
        rng = np.random.default_rng(42)
        peps = []
        for i, p in enumerate(random_peptides(rng, 96, 2, 9, ODD)):
            nterm = [np.nan, 42.010565, -17.026548, 0.0][i % 4]
            mods = np.where(rng.random(len(p.seq)) < 0.4, rng.choice([15.9949, -18.0106, 229.1629, -1.0078], len(p.seq)), 0.0)
            peps.append(Pep(p.seq, mods, nterm, decoy=i % 2, missed=i % 3))
        return database(peps, ALL, min_ion_index)
    return build


def signs(kinds):
    """leading b-ions below zero, an ion of exactly 0.0, y-ions below zero behind a heavy C-terminal modification"""
    def build():
        rng = np.random.default_rng(7)
        peps = random_peptides(rng, 24, 3, 8)
        for p in random_peptides(rng, 8, 3, 8):
            peps.append(Pep(p.seq, [-500.0] + [0.0] * (len(p.seq) - 1)))            # b1, b2, .. < 0 until the residues outweigh it
        for p in random_peptides(rng, 8, 3, 8):
            peps.append(Pep(p.seq, [-RESIDUE_MASS[p.seq[0]]] + [0.0] * (len(p.seq) - 1)))   # b1 == 0.0 exactly
        for p in random_peptides(rng, 4, 3, 6):
            peps.append(Pep(p.seq, [0.0] * (len(p.seq) - 1) + [-900.0], mono=F32(40.0)))     # y-ions < 0 (mass set by hand)
        return database(peps, kinds, 0)
    return build


CELL_EDGE_TOPS = {
    # the database's largest m/z: on an edge of both tables, on an edge of the 1/256 table only (odd k), one ulp either side
    "top_k32": 9000.0 / 32.0, "top_k32_below": np.nextafter(F32(9000.0 / 32.0), F32(0)), "top_k32_above": np.nextafter(F32(9000.0 / 32.0), F32(1e9)),
    "top_k256": 70001.0 / 256.0, "top_k256_below": np.nextafter(F32(70001.0 / 256.0), F32(0)), "top_k256_above": np.nextafter(F32(70001.0 / 256.0), F32(1e9)),
}


def cell_edges(top):
    """two residues, b only, every ion stored: the m/z of the database are exactly the chosen first steps — k / 32 and k / 256 and
    their neighbours one ulp either side, for the first cells, cells in the middle and the table's last cell (`top`)"""
    def build():
        targets = []
        for k32 in (1, 2, 33, 4095):
            e = F32(k32 / 32.0)
            targets += [e, np.nextafter(e, F32(0)), np.nextafter(e, F32(1e9))]
        for k256 in (1, 3, 257, 33331):
            e = F32(k256 / 256.0)
            targets += [e, np.nextafter(e, F32(0)), np.nextafter(e, F32(1e9))]
        targets = [t for t in targets if t < F32(top)] + [F32(top)]
        peps = []
        for i, t in enumerate(targets):
            if i % 2 or t < 128.0:  # through a residue of mass 0 (the only way to the neighbours of a small value) ...
                peps.append(Pep(b"BA", [t, 0.0]))
            else:      # ... and through glycine plus the modification that lands on t
                peps.append(Pep(b"GA", [step_mod(ord("G"), t), 0.0]))
        return database(peps, (KIND_B,), 0)
    return build


def ties():
    """one sequence at several indices — inside a small tile (10..13) and across a seam (60..66, tiles of 64) — and a peptide whose
    b1 and y1 coincide (two equal entries of ONE peptide: its mass is set to twice its first residue's)"""
    rng = np.random.default_rng(99)
    peps = sorted(random_peptides(rng, 130, 3, 10), key=lambda p: float(p.mono))
    for lo, hi, src in ((9, 12, 9), (59, 65, 61)):  # (the light peptide below takes index 0)
        for i in range(lo, hi + 1):
            peps[i] = Pep(peps[src].seq, peps[src].mods, decoy=i % 2)
    peps.append(Pep(b"GGG", mono=F32(G + G)))
    db = database(peps, BY, 0)
    assert db.seq[int(db.seq_off[0]):int(db.seq_off[1])].tobytes() == b"GGG"
    return db


def tiny():
    return database(random_peptides(np.random.default_rng(3), 20, 3, 8))


def empty():
    return database([])


T2 = {"SAGE_HIP_TILE2_SHIFT": "6"}
T1 = {"SAGE_HIP_TILE_SHIFT": "11"}
HAND_BUILT = (
    [(f"seam_small_{n}", T2, seam_small(n)) for n in (63, 64, 65, 129)] +
    [(f"seam_large_{n}", T1, seam_large(n)) for n in (2047, 2048, 2049, 4133)] +
    [("empty_middle", T2, empty_middle)] +
    [(f"lengths_{name}_min{mi}", T2, lengths(kinds, mi)) for name, kinds in (("y", (KIND_Y,)), ("by", BY), ("abcxyz", ALL)) for mi in (0, 2, 5)] +
    [(f"termini_min{mi}", T2, termini(mi)) for mi in (0, 1)] +
    [(f"signs_{name}", T2, signs(kinds)) for name, kinds in (("by", BY), ("abcxyz", ALL))] +
    [(f"cell_edges_{name}", {}, cell_edges(top)) for name, top in CELL_EDGE_TOPS.items()] +
    [("ties", T2, ties), ("tiny", {}, tiny), ("empty", {}, empty)]
)
