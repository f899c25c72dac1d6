"""The guard of tests/rescore_edge_cases.py and two numpy readings of the reference — CPU only, the oracle alone.

The guard keeps the GPU tests of test_gpu_rescore_edges.py honest: a case may leave out the reference-order leg only where the
oracle's own two modes fail that leg against each other, a tie table has ties, a seam table hits its number, a non-finite
table delivers NaN and -inf to the sort.  The readings (q-values and order from the discriminants, the picked competition) are
written from ml/qvalue.rs and fdr.rs, not from the oracle, so that "device == oracle" on ties means something.
"""
import functools
import types

import numpy as np
import pytest

import oracle_lib
from rescore_edge_cases import (CLASS_BLOCK, CLASS_SEAMS, COMPETITION_SEAMS, GRID_TRIP, HEURISTIC_CASES, LDA_SEAM_SIZES, LDA_TILE, NO_KEY,
                                RESCORE_CASES, ROW_TILE, RT_CASES, TIE_CASES, competition_rows, descending_stable_order, picked_q_of,
                                spectrum_q_of)
from test_gpu_rescore import reference_leg

SMALL = [name for name, case in RESCORE_CASES.items() if len(case[0]) <= GRID_TRIP]


@functools.lru_cache(maxsize=None)
def oracle_pair(name):
    """(det=True result with the device's field names, det=False result) of a case — computed once, shared, left unchanged."""
    f, pk, n_pk, prk, n_pr, opt, _ = RESCORE_CASES[name]
    opt = dict(opt)
    tol = opt.pop("tol")
    a = oracle_lib.rescore(f, tol, pk, n_pk, prk, n_pr, det=True, **opt)
    r = oracle_lib.rescore(f, tol, pk, n_pk, prk, n_pr, det=False, want_rows=True, **opt)
    return types.SimpleNamespace(**a), r


def share_tied(values):
    _, inverse, counts = np.unique(np.asarray(values), return_inverse=True, return_counts=True)
    return float(np.mean(counts[inverse] > 1))


# ---- the guard ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RESCORE_CASES))
def test_ref_leg_is_a_fact_about_the_data(name):
    """ref_leg=True: the oracle's det=True output passes, against its det=False output, every assertion compare() applies to
    the device on that leg.  ref_leg=False: it does not (or the table is past 131 072 rows, where an oracle pass costs
    seconds).  Nothing in between: a case whose leg is empty (no fit, a constant column) carries True and is held to the
    fit-or-heuristic decision."""
    n, ref_leg = len(RESCORE_CASES[name][0]), RESCORE_CASES[name][6]
    if n > GRID_TRIP:
        assert not ref_leg
        return
    a, r = oracle_pair(name)
    if ref_leg:
        reference_leg(a, r, name)
    else:
        with pytest.raises(AssertionError):
            reference_leg(a, r, name)


def test_reference_leg_coverage():
    """Each family has cases on which the per-PSM half of the leg really runs; the seam tables of some 3000 rows all do."""
    live = {name for name in SMALL if RESCORE_CASES[name][6] and reference_leg(*oracle_pair(name), name)}
    for family in ("tie/", "lda_seam/", "class_seam/", "comp_seam/", "da/"):
        assert any(name.startswith(family) for name in live), family
    assert {"tie/repeat3", "tie/twins", "da/repeat3"} <= live
    assert {f"lda_seam/n{n}" for n, _, _ in LDA_SEAM_SIZES if n >= LDA_TILE // 2 - 1} <= live  # (n <= 3: no fit, the leg is empty)
    assert set(CLASS_SEAMS) | set(COMPETITION_SEAMS) | {"da/class_seam_d1025_t1977"} <= live


def test_tie_tables_have_ties():
    for name in TIE_CASES:
        a, _ = oracle_pair(name)
        assert share_tied(a.discriminant_score.view(np.uint32)) >= 0.6, name
    # the twin table: keys whose best target and best decoy are the same f32
    f, pk, n_pk, *_ = RESCORE_CASES["tie/twins"]
    a, _ = oracle_pair("tie/twins")
    decoy = f["label"] == -1
    best = np.full((n_pk, 2), -np.inf, np.float32)
    np.maximum.at(best, (pk.astype(np.int64), decoy.astype(np.int64)), a.discriminant_score)
    equal = best[:, 0].view(np.uint32) == best[:, 1].view(np.uint32)
    assert equal.sum() >= 100 and (~equal).sum() >= 100
    assert a.lda_fitted and a.passing[0] > 0  # ... and something still passes 1 %
    assert share_tied(RT_CASES["rt/quantised_poisson"][0]["poisson"]) >= 0.5


def test_heuristic_tables_take_the_heuristic_path():
    for name in HEURISTIC_CASES:
        a, r = oracle_pair(name)
        assert not a.lda_fitted and not r["lda_fitted"], name
    assert (RESCORE_CASES["tie/quantised_poisson"][0]["label"] == -1).any()  # (not for want of decoys)


def test_seam_tables_hit_their_numbers():
    assert [n for n, _, _ in LDA_SEAM_SIZES] == [1, 2, 3, LDA_TILE // 2 - 1, LDA_TILE // 2, LDA_TILE // 2 + 1, LDA_TILE - 1, LDA_TILE,
                                                 LDA_TILE + 1, 2 * LDA_TILE - 1, 2 * LDA_TILE, 2 * LDA_TILE + 1, 3 * LDA_TILE - 1,
                                                 3 * LDA_TILE + 1]
    for n, _, _ in LDA_SEAM_SIZES:
        assert len(RESCORE_CASES[f"lda_seam/n{n}"][0]) == len(RESCORE_CASES[f"lda_seam_const/n{n}"][0]) == n
    at_seam = (CLASS_BLOCK - 1, CLASS_BLOCK, CLASS_BLOCK + 1)
    seen = set()
    for name, (n_d, n_t, _) in dict(CLASS_SEAMS, **{"da/class_seam_d1025_t1977": (1025, 1977, None)}).items():
        label = RESCORE_CASES[name][0]["label"]
        assert (int((label == -1).sum()), int((label == 1).sum())) == (n_d, n_t) and len(label) == n_d + n_t, name
        assert (n_d in at_seam) != (n_t in at_seam) and (n_t if n_d in at_seam else n_d) % CLASS_BLOCK != 0, name
        seen.add(("decoys", n_d) if n_d in at_seam else ("targets", n_t))
    assert seen == {(side, k) for side in ("decoys", "targets") for k in at_seam}
    for name, (m_pep, m_prot, _) in COMPETITION_SEAMS.items():
        f, pk, _, prk, _, _, _ = RESCORE_CASES[name]
        decoy = f["label"] == -1
        assert (competition_rows(pk, decoy), competition_rows(prk, decoy)) == (m_pep, m_prot), name
    tiles = (ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 2 * ROW_TILE, 2 * ROW_TILE + 1)
    assert sorted(m for m, _, _ in COMPETITION_SEAMS.values()) == list(tiles)
    assert sorted(m for _, m, _ in COMPETITION_SEAMS.values()) == [1, 2, ROW_TILE - 1, ROW_TILE + 1, 2 * ROW_TILE]
    # past one trip of the grid-stride reductions, both extremes of the mass error in the second trip
    dm = RESCORE_CASES["grid_seam/n131372"][0]["delta_mass"]
    assert len(dm) == GRID_TRIP + 300 and np.argmax(dm) >= GRID_TRIP and np.argmin(dm) >= GRID_TRIP
    assert dm[:GRID_TRIP].max() < dm.max() and dm[:GRID_TRIP].min() > dm.min()


def test_nonfinite_tables_deliver_nan_and_minus_inf_to_the_sort():
    a, _ = oracle_pair("nonfinite/poisson")
    d = a.discriminant_score
    assert np.isnan(d).sum() == 3 and np.isneginf(d).sum() == 1
    # a non-finite entry of the design: the sums of the fit are NaN, no model, heuristic discriminants (all finite)
    for name in ("nonfinite/hyperscore_nan", "nonfinite/hyperscore_inf", "nonfinite/delta_mass_nan", "nonfinite/ims_inf",
                 "nonfinite/rt_inf"):
        a, r = oracle_pair(name)
        assert not a.lda_fitted and not r["lda_fitted"] and np.isfinite(a.discriminant_score).all(), name
    # ... while these two are ordinary inputs: hyperscore 0 is ln_1p(0), ms2_intensity is no column of the design
    for name in ("nonfinite/hyperscore_zero", "nonfinite/ms2_intensity_inf"):
        assert oracle_pair(name)[0].lda_fitted, name


def test_degenerate_competitions_are_what_they_say():
    f, pk, n_pk, prk, n_pr, _, _ = RESCORE_CASES["degenerate/all_proteins_shared"]
    assert n_pr == 0 and np.all(prk == NO_KEY) and np.all(oracle_pair("degenerate/all_proteins_shared")[0].protein_q == 1.0)
    f, pk, n_pk, prk, n_pr, _, _ = RESCORE_CASES["degenerate/one_key"]
    assert (n_pk, n_pr) == (1, 1) and not pk.any() and not prk.any()
    f, pk, n_pk, prk, n_pr, _, _ = RESCORE_CASES["degenerate/one_sided_keys"]
    decoy = f["label"] == -1
    assert competition_rows(pk, decoy) == n_pk and competition_rows(prk, decoy) == n_pr
    for name, decoys in (("degenerate/one_decoy", 1), ("degenerate/one_target", 2999), ("degenerate/all_decoys", 3000)):
        assert int((RESCORE_CASES[name][0]["label"] == -1).sum()) == decoys, name


def test_rt_cases_are_what_they_say():
    o = {name: oracle_lib.predict_rt(*case) for name, case in RT_CASES.items()}
    for name in ("rt/n1", "rt/n2", "rt/n70"):
        assert not o[name]["fitted"].any(), name
    assert o["rt/n257"]["fitted"].all()
    f, n_files, *_ = RT_CASES["rt/files70"]
    assert n_files == 70 and len(np.unique(f["file_id"])) == 70 and o["rt/files70"]["fitted"].all()
    f, n_files, *_ = RT_CASES["rt/unused_file_id"]
    assert n_files == int(f["file_id"].max()) + 2 and o["rt/unused_file_id"]["alignments"][-1, 0] == 0.0
    z = o["rt/zero_rt_file"]
    f = RT_CASES["rt/zero_rt_file"][0]
    assert z["alignments"][1, 0] == 0.0 and np.isnan(z["aligned_rt"][f["file_id"] == 1]).all() and np.isnan(z["r2"][0])
    assert np.isfinite(z["aligned_rt"][f["file_id"] != 1]).all()
    s = o["rt/rt_specials"]
    assert s["alignments"][0, 0] == np.float32(2.0 ** 32) and 0 < s["alignments"][1, 0] < 1000.0
    assert np.isnan(s["aligned_rt"]).sum() == 1 and np.isinf(s["aligned_rt"]).sum() == 1
    seq = RT_CASES["rt/odd_residues"][3]
    assert all((seq == ord(c)).sum() > 100 for c in "XBU") and np.all((seq >= ord("A")) & (seq <= ord("Z")))
    f = RT_CASES["rt/one_file_per_peptide"][0]
    pairs = np.unique(np.stack([f["peptide_idx"], f["file_id"]], 1), axis=0)
    assert len(pairs) == len(np.unique(f["peptide_idx"])) and len(np.unique(f["file_id"])) == 2


# ---- independent readings ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TIE_CASES + ("nonfinite/poisson",))
def test_order_and_spectrum_q_from_the_discriminants(name):
    """runner.rs:290 + ml/qvalue.rs on the oracle's discriminants: descending f32 total order, ascending row index inside a tie
    (the contract where the reference's unstable sort leaves it open), q-values from the decoy / target counts."""
    a, _ = oracle_pair(name)
    decoy = RESCORE_CASES[name][0]["label"] == -1
    order = descending_stable_order(a.discriminant_score)
    assert np.array_equal(a.order, order)
    assert np.array_equal(a.spectrum_q, spectrum_q_of(order, decoy))


def kde_of_winners(winner, winner_decoy, queries):
    return oracle_lib.kde(winner, winner_decoy.astype(np.uint8), True, 1000, 1.0, queries, det=True)[3]


@pytest.mark.parametrize("name", ["tie/twins", "degenerate/one_sided_keys", "tie/quantised_poisson", "nonfinite/poisson",
                                  "comp_seam/pep1025_prot2048"])
def test_picked_competition_from_the_discriminants(name):
    """fdr.rs:42-120 in numpy on the oracle's discriminants: per-key maxima per side, the decoy wins a tie, rows in key order
    with forward before reverse, stable descending sort, running f32 `decoy += pep`, reverse cumulative minimum, write-back."""
    f, pk, n_pk, prk, n_pr, _, _ = RESCORE_CASES[name]
    a, _ = oracle_pair(name)
    decoy = f["label"] == -1
    assert np.array_equal(a.peptide_q, picked_q_of(pk, n_pk, decoy, a.discriminant_score, kde_of_winners), equal_nan=True)
    assert np.array_equal(a.protein_q, picked_q_of(prk, n_pr, decoy, a.discriminant_score, kde_of_winners), equal_nan=True)
