"""GPU parity of sage_hip_rescore / sage_hip_predict_rt with the CPU oracle on the inputs of tests/rescore_edge_cases.py: ties,
block and tile seams, non-finite values, degenerate competitions.  Same helpers and bounds as tests/test_gpu_rescore.py: bit
equality with the oracle's det=True mode (2.5e-7 relative on posterior_error), compare()'s thresholds against its det=False
mode where the case carries that leg (tests/test_rescore_edges_cpu.py holds every such flag to the data), compare_rt()'s
bounds for the RT block (per world, from profiles/rt_model_spread.json), with NaN required to meet NaN.  On the tie tables the device's own outputs are also read with numpy
restatements of ml/qvalue.rs and fdr.rs that do not go through the oracle."""
import numpy as np
import pytest

import oracle_lib
from rescore_edge_cases import RESCORE_CASES, RT_CASES, TIE_CASES, descending_stable_order, picked_q_of, spectrum_q_of
from test_gpu_rescore import compare, compare_rt, rt_spread

pytestmark = pytest.mark.gpu

PICKED_READINGS = ("tie/twins", "degenerate/one_sided_keys", "tie/quantised_poisson", "nonfinite/poisson", "comp_seam/pep1025_prot2048")


def kde_of_winners(winner, winner_decoy, queries):
    return oracle_lib.kde(winner, winner_decoy.astype(np.uint8), True, 1000, 1.0, queries, det=True)[3]


@pytest.mark.parametrize("name", list(RESCORE_CASES))
def test_rescore_edge_case(gpu_required, name):
    f, pk, n_pk, prk, n_pr, opt, ref_leg = RESCORE_CASES[name]
    opt = dict(opt)
    g, o = compare(f, opt.pop("tol"), pk, n_pk, prk, n_pr, name, ref_leg=ref_leg, **opt)
    decoy = f["label"] == -1
    if name in TIE_CASES or name in PICKED_READINGS:
        # the device's own discriminants -> its own order and q-values, by numpy: stable descending total order, counts
        order = descending_stable_order(g.discriminant_score)
        assert np.array_equal(g.order, order), name
        assert np.array_equal(g.spectrum_q, spectrum_q_of(order, decoy)), name
    if name in PICKED_READINGS:
        # ... and its picked competitions (the KDE of the winners from the oracle's kde(): the device's differs from it in the
        # last bits of posterior_error at most — where that moves a q-value, compare() above has already failed)
        assert np.array_equal(g.peptide_q, picked_q_of(pk, n_pk, decoy, g.discriminant_score, kde_of_winners), equal_nan=True), name
        assert np.array_equal(g.protein_q, picked_q_of(prk, n_pr, decoy, g.discriminant_score, kde_of_winners), equal_nan=True), name


@pytest.mark.parametrize("name", list(RT_CASES))
def test_predict_rt_edge_case(gpu_required, name):
    compare_rt(*RT_CASES[name], name, rt_spread(name))
