"""sage_hip_predict_rt on the order-free worlds of tests/rt_model_worlds.py: the device's retention / mobility model, bit for bit.

On these worlds every sum of X^T X and X^T y is exact in f64 in any order (tests/test_rt_model_cpu.py holds the budget with the
oracle alone), so xtx_kernel's blocked, staged sums are the reference's sequential ones, the host gauss_solve gets the oracle's
input, and every prediction must EQUAL the oracle's (oracle/rescore_oracle.cpp) and the second reading's
(tests/rt_model_reference.py).  Training rows sit on the seams of fit_and_predict's launch: the first and last row of a block,
of a 16-row stage, of the last (partial) block, of predict_kernel's 64-row blocks.  A row lost or counted twice there, a wrong
cterm branch of an embedding for the lengths 1 - 4, or a contraction in the prediction changes bits here while it stays inside
compare_rt()'s bounds on the worlds with noise.

The alignment in front of the models is not order-free (its sum of squares starts from 1e-8), but slope and intercept are f32
casts of f64 values that differ by a relative 1e-15 or so between the two sides: equality is expected, and the retention model's
target depends on it."""
import numpy as np
import pytest

import rt_model_reference as R
import rt_model_worlds as W
from test_gpu_rescore import compare_rt

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", W.WORLD_NAMES)
def test_rt_model_exact(gpu_required, name):
    w, o, r = R.readings(name)
    g, o2 = compare_rt(*w.case, name)  # every field at compare_rt's bounds, NaN meeting NaN
    pred, delta, k = R.model_fields(w.kind)
    assert np.array_equal(o2[pred], o[pred])  # (the oracle is a function of its input)
    got_pred, got_delta = (g.predicted_rt, g.delta_rt_model) if w.kind == "rt" else (g.predicted_ims, g.delta_ims_model)
    got_fitted, got_r2 = ((g.rt_fitted, g.ims_fitted)[k], (g.rt_r2, g.ims_r2)[k])
    for other, src in (("oracle", dict(spectrum_q=o["spectrum_q"], alignments=o["alignments"], aligned_rt=o["aligned_rt"],
                                       predicted=o[pred], delta=o[delta], fitted=bool(o["fitted"][k]))), ("second reading", r)):
        ctx = (name, other)
        assert np.array_equal(g.spectrum_q, src["spectrum_q"]), ctx
        for j, field in enumerate(("max_rt", "slope", "intercept")):
            assert np.array_equal(_bits(g.alignments[field]), _bits(src["alignments"][:, j])), (ctx, field, g.alignments[field], src["alignments"][:, j])
        bad = np.flatnonzero(_bits(g.aligned_rt) != _bits(src["aligned_rt"]))
        assert len(bad) == 0, (ctx, "aligned_rt", len(bad), bad[:5], g.aligned_rt[bad[:5]], src["aligned_rt"][bad[:5]])
        assert bool(got_fitted) == src["fitted"], (ctx, "fitted")
        bad = np.flatnonzero(_bits(got_pred) != _bits(src["predicted"]))
        assert len(bad) == 0, (ctx, pred, len(bad), bad[:5], got_pred[bad[:5]], src["predicted"][bad[:5]],
                               float(np.abs(got_pred.astype(np.float64) - src["predicted"]).max()))
        bad = np.flatnonzero(_bits(got_delta) != _bits(src["delta"]))
        assert len(bad) == 0, (ctx, delta, len(bad), bad[:5])
    assert (bool(g.rt_fitted), bool(g.ims_fitted)) == tuple(bool(x) for x in o["fitted"]), name
    if got_fitted and np.isfinite(o["r2"][k]):
        # im worlds with more than one distinct ims: y_var is exact, only the SSE sum has an order; else compare_rt's 1e-5 stands
        exact_var = w.kind == "im" and len(np.unique(w.case[0]["ims"][w.train])) > 1
        tol = 1e-12 * abs(o["r2"][k]) if exact_var else 1e-5
        assert abs(got_r2 - o["r2"][k]) <= tol and abs(got_r2 - r["r2"]) <= tol, (name, got_r2, o["r2"][k], r["r2"])
