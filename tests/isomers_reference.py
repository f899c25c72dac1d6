"""Plain restatements for positional-isomer scoring — TEST INFRASTRUCTURE.

The grouping restates the definition: two peptides of a host database are positional isomers when their decoy flag, their
residue bytes and the multiset of their modification masses (bit patterns of the non-zero entries of `mods`, of nterm and of
cterm when neither NaN nor 0) are equal.  The scoring is tests/second_reading.py's SecondScorer.score_candidate and
.remove_matched_peaks, imported, not copied.
"""
import numpy as np

import second_reading as SR
from sage_amd import _lib as L

NONE = 0xFFFFFFFF

# the database of the issue's measurement: C3's settings plus phospho S/T/Y, oxidation and the peptide N-terminal acetylation
VARMODS = {"M": [15.9949], "S": [79.9663], "T": [79.9663], "Y": [79.9663], "[": [42.010565]}
ENZYME = dict(missed_cleavages=1, min_len=5, max_len=50, cleave_at="KR", restrict="P")
PHOSPHO_DB = dict(bucket_size=8192, peptide_min_mass=500.0, peptide_max_mass=5000.0, static_mods={"C": 57.0215},
                  generate_decoys=True, enzyme=ENZYME, variable_mods=VARMODS, max_variable_mods=2)


def isomer_groups(db):
    """(group_of[n_peptides] u32, group_off[n_groups + 1] u64, members u32) of anything with the flat peptide arrays of
    sage_amd.api.IndexedDatabase: groups of at least two, numbered by ascending smallest member, members ascending."""
    seq_off = np.asarray(db.seq_off).astype(np.int64)
    by_key = {}
    for p in range(len(seq_off) - 1):
        a, b = seq_off[p], seq_off[p + 1]
        m = np.asarray(db.mods[a:b], dtype=np.float32)
        masses = [int(x) for x in m[m != 0].view(np.uint32)]
        for t in (np.float32(db.nterm[p]), np.float32(db.cterm[p])):
            if not np.isnan(t) and t != 0:
                masses.append(int(t.view(np.uint32)))
        by_key.setdefault((int(db.decoy[p]), bytes(db.seq[a:b]), tuple(sorted(masses))), []).append(p)
    groups = sorted((v for v in by_key.values() if len(v) >= 2), key=lambda v: v[0])
    group_of = np.full(len(seq_off) - 1, NONE, dtype=np.uint32)
    group_off = np.zeros(len(groups) + 1, dtype=np.uint64)
    members = []
    for g, v in enumerate(groups):
        assert v == sorted(v)
        group_of[v] = g
        members += v
        group_off[g + 1] = len(members)
    return group_of, group_off, np.array(members, dtype=np.uint32)


def second_scorer(host, dbp, params):
    """SecondScorer over the peptides of a sage_amd.api.IndexedDatabase"""
    arrays = dict(pep_mono=host.pep_mono, seq_off=host.seq_off, seq=host.seq, mods=host.mods, nterm=host.nterm, decoy=host.decoy,
                  missed=host.missed_cleavages)
    kinds = [L.ION_KINDS[k] for k in (dbp.ion_kinds if dbp.ion_kinds is not None else ["b", "y"])]
    return SR.SecondScorer(SR.Peptides(arrays), kinds, 2 if dbp.min_ion_index is None else dbp.min_ion_index, params)


def others(groups, pep):
    """every other member of pep's group, ascending"""
    group_of, group_off, members = groups
    g = int(group_of[pep])
    if g == NONE:
        return []
    return [int(m) for m in members[int(group_off[g]):int(group_off[g + 1])] if int(m) != pep]


def score(sr, masses, intensities, pep, charge):
    """score_candidate's Score as a SageCandidateScore-shaped dict"""
    s = sr.score_candidate(masses, intensities, (0, int(pep), int(charge), 0))
    return dict(hyperscore=s["hyperscore"], summed_b=s["summed_b"], summed_y=s["summed_y"], average_ppm=s["ppm_difference"],
                matched_b=s["matched_b"], matched_y=s["matched_y"], longest_b=s["longest_b"], longest_y=s["longest_y"])


def states(sr, masses, intensities, psms):
    """The spectrum as PSM r was scored in, for every r: with chimera, after remove_matched_peaks of PSMs 0 .. r-1.
    psms: [(peptide_idx, charge)] in rank order."""
    out = []
    for pep, z in psms:
        out.append((masses, intensities))
        if sr.p.chimera:
            masses, intensities, _ = sr.remove_matched_peaks(masses, intensities, dict(peptide_idx=int(pep), charge=int(z)))
    return out


INT_FIELDS = ["matched_b", "matched_y", "longest_b", "longest_y"]
F32_FIELDS = ["summed_b", "summed_y", "average_ppm"]


def assert_score_equal(got, want, f64_tol, ctx):
    """Integers and f32 bit for bit (NaN == NaN), hyperscore as tests/test_scoring_second_reading.py compares f64 fields."""
    for k in INT_FIELDS:
        assert int(got[k]) == int(want[k]), f"{ctx}: {k}: device {got[k]} vs second reading {want[k]}"
    for k in F32_FIELDS:
        a, b = np.float32(got[k]), np.float32(want[k])
        assert a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b)), f"{ctx}: {k}: device {a!r} vs second reading {b!r}"
    a, b = float(got["hyperscore"]), float(want["hyperscore"])
    assert abs(a - b) <= f64_tol * max(abs(b), 1.0), f"{ctx}: hyperscore: device {a!r} vs second reading {b!r}"


def pick_best(peps, hypers):
    """largest hyperscore under a plain `>`; ties to the smallest peptide index (peps ascending)"""
    best = 0
    for j in range(1, len(peps)):
        if hypers[j] > hypers[best]:
            best = j
    return peps[best], best
