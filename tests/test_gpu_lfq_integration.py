"""integrate_kernel's decisions on drawn traces, and the parameters of sage_hip_lfq that had only ever had one value.

Named cases (tests/lfq_traces.py): every case is a tiny world whose grid is drawn through MS1 peaks so that one decision of
Traces::integrate is reached on purpose — a silent file, shifts of 74 / 75 / -75 / 76 bins, two exactly equal offsets, a
reference file other than 0, a plateau wider than 40 bins, peaks at both grid ends, two exactly equal scores, a bound walk
stopped by the angle threshold, a threshold that fails everywhere, a trace exactly proportional to the isotope distribution,
1 / 2 / 9 files, two charge states, a decoy twin.  Each has asserted its defining property on the restatement before the device
is asked.  The device is compared under peak_scoring x spectral_angle {0.70, 0.0} x integration {Sum, Apex}, with
combine_charge_states both ways where a case has two charge states, by two routes:
  - test_gpu_lfq.assert_same against tests/lfq_reference.py (matrix bits, warps, has_peak, bin, bounds, area bits, q-values;
    score and angle within ULPS);
  - the device's own debug matrices through tests/lfq_second_reading.py, which never passes through lfq_reference.py.
Combinations in lfq_traces.FRAGILE (tests/test_lfq_integration_cpu.py) are compared for matrix and warps only.

Twelve small worlds from synthetic_lcms vary together what every earlier LFQ test held fixed: the file count, the charge
range, the ppm tolerance, the alignments, the reference file, the shape and order of the MS1 batches, special intensities."""
import numpy as np
import pytest

import lfq_reference as R
import lfq_second_reading as S2
import lfq_traces as T
from sage_amd.api import LfqSettings, lfq, lfq_im
from test_gpu_lfq import ULPS, assert_same, ulp_close

pytestmark = pytest.mark.gpu

assert ULPS == T.ACOS_ULPS


@pytest.fixture(scope="module")
def db():
    return T.database()


def device(world, settings, charge, im=False):
    st = LfqSettings(peak_scoring=settings["peak_scoring"], integration=settings["integration"],
                     spectral_angle=settings["spectral_angle"], ppm_tolerance=settings["ppm_tolerance"],
                     mobility_pct_tolerance=settings["mobility_pct_tolerance"], combine_charge_states=settings["combine_charge_states"])
    call = lfq_im if im else lfq
    return call(world["f"], None, world["art"], world["pq"], world["al"], world["batches"], world["carbon"], world["sulfur"], st,
                charge, debug=True)


def assert_matrix_and_warps(dev, ref, grids):
    keys = [(int(p), int(z), bool(d)) for p, z, d in zip(dev.peptide_idx, dev.charge, dev.decoy)]
    assert keys == sorted(grids), "grid keys"
    for i, k in enumerate(keys):
        np.testing.assert_array_equal(dev.matrix[i].view(np.uint64), grids[k]["matrix"].view(np.uint64), err_msg=f"matrix {k}")
        assert dev.warps[i].tolist() == ref[k]["warps"], k


def assert_second_reading(db, dev, reference_file, settings, decisions=True):
    """the device's outputs against the second reading of its own matrices: exact, but score and angle within ULPS"""
    iso = T.isotopes_of(db)
    rows = []
    for i in range(len(dev.peptide_idx)):
        p = int(dev.peptide_idx[i])
        want = S2.integrate(dev.matrix[i], iso(p), reference_file[p], settings)
        k = (p, int(dev.charge[i]), bool(dev.decoy[i]))
        assert dev.warps[i].tolist() == want["warps"], k
        if not decisions:
            continue
        assert bool(dev.has_peak[i]) == want["peak"], k
        if not want["peak"]:
            continue
        assert (int(dev.peak_rt[i]), int(dev.left[i]), int(dev.right[i])) == (want["rt"], want["left"], want["right"]), k
        np.testing.assert_array_equal(dev.areas[i].view(np.uint64), np.array(want["areas"]).view(np.uint64), err_msg=f"areas {k}")
        assert ulp_close(dev.score[i], want["score"]) and ulp_close(dev.spectral_angle[i], want["spectral_angle"]), \
            (k, dev.score[i], want["score"], dev.spectral_angle[i], want["spectral_angle"])
        rows.append(i)
    if decisions and rows:  # picked_precursor on the device's own scores, in grid order
        q, passing = S2.picked_precursor(dev.decoy[rows] != 0, dev.score[rows])
        assert dev.q_value[rows].tolist() == q.tolist() and dev.passing == passing


# ---- the named cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.CASES)
def test_named_case(db, name):
    world = T.case(db, name)
    n_files = world["n_files"]
    seen = 0
    for combine, grids in world["grids"].items():
        for scoring in R.SCORING:
            for thr in T.THRESHOLDS:
                for integration in R.INTEGRATION:
                    settings = R.default_settings(peak_scoring=scoring, spectral_angle=thr, integration=integration,
                                                  combine_charge_states=combine, ppm_tolerance=world["ppm"])
                    ref, passing, _ = R.quantify(settings, T.CHARGES, None, None, None, n_files, None, grids=grids)
                    dev = device(world, settings, T.CHARGES)
                    assert dev.n_windows == len(world["fmap"]["ranges"])
                    robust = (name, scoring, thr) not in T.FRAGILE
                    if robust:
                        assert_same(dev, ref, grids, passing, n_files)
                        # the grids without a peak keep the q-value they were given
                        assert all(q == 1.0 for q, has in zip(dev.q_value, dev.has_peak) if not has)
                    else:
                        assert_matrix_and_warps(dev, ref, grids)
                    assert_second_reading(db, dev, world["ref"], settings, decisions=robust)
                    seen += 1
    assert seen == 16 * len(world["grids"])


# ---- parameters that have only ever had one value -------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(T.N_WORLDS))
def test_parameter_world(db, i):
    world = T.param_world(db, i)
    n_files, charge, combine, ppm, im, settings = T.param_settings(i)
    dev = device(world, settings, charge, im=im)
    assert dev.n_windows == len(world["fmap"]["ranges"]) == len(np.unique(world["f"]["peptide_idx"])) * (charge[1] - charge[0] + 1) * 6
    assert dev.matrix.shape[1:] == (n_files * 3, 100) and dev.areas.shape[1] == n_files == dev.warps.shape[1]
    assert_same(dev, world["ref"], world["grids"], world["passing"], n_files)
    reference_file = {int(p): int(f) for p, f in zip(world["f"]["peptide_idx"], world["f"]["file_id"])}
    assert_second_reading(db, dev, reference_file, settings)
