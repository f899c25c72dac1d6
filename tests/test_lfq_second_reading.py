"""The two readings of label-free quantification's integration stage held equal, bit for bit (NaN = NaN), without a GPU:
tests/lfq_reference.py (the checker of sage_hip_lfq, sequential) against tests/lfq_second_reading.py (written from lfq.rs
alone, whole arrays).  On every drawn case of tests/lfq_traces.py, on the matrices of test_gpu_lfq.py's synthetic run, and on
2 000 seeded random matrices fed straight in — lobes, plateaus, zero rows, rows of one repeated value, 5 % with an inf or a NaN
cell, where both must agree on whatever lfq.rs does with it."""
import numpy as np
import pytest

import lfq_reference as R
import lfq_second_reading as S2
import lfq_traces as T

THRESHOLDS = (0.70, 0.0)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def assert_readings_equal(first, second, what):
    assert first["warps"] == second["warps"], (what, first["warps"], second["warps"])
    assert first["peak"] == second["peak"], what
    if not first["peak"]:
        return
    assert (first["rt"], first["left"], first["right"]) == (second["rt"], second["left"], second["right"]), what
    for k in ("areas", "score", "spectral_angle"):
        assert same_bits(first[k], second[k]), (what, k, first[k], second[k])


def both(matrix, dist, ref, settings):
    grid = dict(matrix=np.array(matrix, dtype=np.float64), dist=np.asarray(dist, np.float32), ref=ref)
    return R.integrate(grid, settings), S2.integrate(matrix, dist, ref, settings)


def test_kernel_and_rt_factor_tables():
    assert same_bits(R.gaussian_kernel(0.5, R.K_WIDTH), S2.kernel())
    assert same_bits(R.rt_factor_table(), S2._RT_POW)


# ---- random matrices ---------------------------------------------------------------------------------------------------------
def random_matrix(rng):
    files = int(rng.choice([1, 2, 3, 5, 9]))
    dist = np.array([1.0, rng.uniform(0.3, 1.0), rng.uniform(0.05, 0.6)], np.float32)
    dist = dist / dist.max()
    m = np.zeros((files * 3, 100))
    x = np.arange(100.0)
    for f in range(files):
        kind = rng.choice(["lobe", "lobes", "plateau", "zero", "flat", "noise"], p=[0.35, 0.2, 0.15, 0.1, 0.1, 0.1])
        if kind == "zero":
            continue
        if kind == "flat":  # rows of one repeated value (per isotope the same value in every bin)
            prof = np.full(100, float(rng.choice([1.0, 3.0, 1e6, 1e-3])))
        elif kind == "plateau":
            a = int(rng.integers(0, 60))
            prof = np.zeros(100)
            prof[a:a + int(rng.integers(20, 80))] = float(rng.choice([1.0, 1024.0, 3e5]))
        elif kind == "noise":
            prof = rng.lognormal(8.0, 1.0, 100) * (rng.random(100) < 0.3)
        else:
            prof = np.zeros(100)
            for _ in range(1 if kind == "lobe" else int(rng.integers(2, 4))):
                prof += rng.lognormal(12.0, 1.5) * np.exp(-0.5 * ((x - rng.uniform(-10, 110)) / rng.uniform(0.8, 15.0)) ** 2)
        wrong = rng.random() < 0.15  # an isotope pattern that is not the peptide's
        for iso in range(3):
            scale = float(dist[iso]) * (1.0 + 0.05 * rng.normal()) if not wrong else float(rng.random())
            m[f * 3 + iso] = prof * scale if kind != "flat" else prof
        if rng.random() < 0.1:  # the negative cell an interp < 0 leaves behind
            m[f * 3 + int(rng.integers(0, 3)), int(rng.integers(0, 100))] *= -0.5
    if rng.random() < 0.05:
        m[int(rng.integers(0, files * 3)), int(rng.integers(0, 100))] = rng.choice([np.inf, -np.inf, np.nan])
    settings = R.default_settings(peak_scoring=str(rng.choice(R.SCORING)), integration=str(rng.choice(R.INTEGRATION)),
                                  spectral_angle=float(rng.choice(THRESHOLDS)))
    return m, dist, int(rng.integers(0, files)), settings


def test_random_matrices_both_readings_bit_equal():
    rng = np.random.default_rng(20240611)
    peaks = nonfinite = 0
    seen_files, seen_warps = set(), set()
    for n in range(2000):
        m, dist, ref, settings = random_matrix(rng)
        first, second = both(m, dist, ref, settings)
        assert_readings_equal(first, second, (n, settings["peak_scoring"], settings["spectral_angle"], settings["integration"]))
        peaks += first["peak"]
        nonfinite += not np.isfinite(m).all()
        seen_files.add(m.shape[0] // 3)
        seen_warps.update(first["warps"])
    # the draw reaches what it is meant to reach
    assert seen_files == {1, 2, 3, 5, 9} and 60 <= nonfinite <= 140 and 800 <= peaks <= 1900, (seen_files, nonfinite, peaks)
    assert {-75, 0, 75} <= seen_warps and len(seen_warps) > 60


def test_picked_precursor_both_readings():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 7, 40, 300):
        for trial in range(6):
            decoy = rng.random(n) < rng.choice([0.0, 0.1, 0.5, 1.0])
            score = rng.choice([0.25, 0.5, 1.0, 1.5], n) if trial % 2 else rng.random(n) * 3
            if n > 2 and trial == 3:
                score[:2] = [np.inf, 1e-320]
            keys = [(i, 0, bool(d)) for i, d in enumerate(decoy)]
            q1, p1 = R.picked_precursor(list(zip(keys, score.tolist())))
            q2, p2 = S2.picked_precursor(decoy, score)
            assert p1 == p2 and [q1[k] for k in keys] == q2.tolist(), (n, trial)


# ---- the drawn cases and the synthetic run ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def db():
    return T.database()


@pytest.mark.parametrize("name", T.CASES)
def test_drawn_cases_both_readings_bit_equal(db, name):
    world = T.case(db, name)
    n = 0
    for combine, grids in world["grids"].items():
        for key, g in grids.items():
            for scoring in R.SCORING:
                for thr in THRESHOLDS:
                    for integration in R.INTEGRATION:
                        st = R.default_settings(peak_scoring=scoring, spectral_angle=thr, integration=integration)
                        first, second = both(g["matrix"], g["dist"], g["ref"], st)
                        assert_readings_equal(first, second, (name, combine, key, scoring, thr, integration))
                        n += 1
    assert n >= 16


def test_synthetic_run_both_readings_bit_equal(db):
    run = T.run_world(db)
    fmap = R.build_feature_map(R.default_settings(), (2, 4), T.ref_feats(run["f"], run["art"], run["pq"]))
    peaks = 0
    for combine in (True, False):
        grids = R.trace(fmap, run["spectra"], run["alignments"], 3, combine, T.isotopes_of(db))
        assert len(grids) > 20
        for key, g in grids.items():
            for scoring in R.SCORING:
                st = R.default_settings(peak_scoring=scoring)
                first, second = both(g["matrix"], g["dist"], g["ref"], st)
                assert_readings_equal(first, second, (key, scoring))
                peaks += first["peak"]
    assert peaks > 100
