"""The tracing half of label-free quantification without a device: the multi-page worlds of tests/lfq_trace_worlds.py hold
what they were built for, and two readings of the tracing pass agree on them bit for bit.

  - test_census: per world, lfq_trace_worlds.census — the page count, a matched window in every page, both sides of the
    seams, a spectrum that matches in three or more pages, the spectra a tolerance from the shared min_rt, the one-ulp-outside
    peaks, cells whose sum depends on the order of their additions, the last row of the last grid slot — asserted on the
    brute force's matches alone.  Conditions, not measurements: a world that misses one gets another seed or draw.  Then
    lfq_trace_bruteforce.match_pruned, which the GPU test uses, against the exhaustive match: the same matches in the same order.
  - test_pages_are_the_restatements: the pages the census speaks of are the pages lfq_reference.build_feature_map cuts.
  - test_brute_force_equals_restatement: lfq_trace_bruteforce.trace (no pages, no sort, no search) against
    lfq_reference.trace (lfq_im_reference.trace for p5), grid keys and every matrix as uint64 bits: on all spectra of p1 and
    p2, and on every seam spectrum of the larger worlds (on a page's min_rt, across a seam, a tolerance from the shared
    min_rt) plus the last-slot spectrum, the near-zero ones and three in four of the rest.
  - test_existing_worlds: the same comparison on the earlier small worlds wherever require_layout_free accepts the map —
    lfq_traces.run_world and param_world(i) — and the list of those it refuses, which is exact: REFUSED.

Measured on a CPU-only machine: this file 44 s, of which test_existing_worlds 6 s (the twelve param_worlds' construction, which
a whole-suite run shares with tests/test_lfq_integration_cpu.py, included); tests/test_lfq_second_reading.py at the parent
commit 79 s.  The subsets are three quarters of the larger worlds' spectra at that."""
import numpy as np
import pytest

import lfq_im_reference as RI
import lfq_reference as R
import lfq_trace_bruteforce as B
import lfq_trace_worlds as W
import lfq_traces as T

# param_world(i) whose map require_layout_free refuses: the three 50 ppm worlds, all of which hold charge 1 (a window at mass m
# is 1e-4 m wide: 0.1 from 1000 Da).  At 20 ppm a window reaches 0.1 from 2500 Da, which no window of these worlds does.
REFUSED = (3, 6, 9)


def _restatement(wd, subset=None):
    sp = wd["spec"]
    if "fmap" not in wd["cache"]:
        feats = T.ref_feats(wd["f"], wd["art"], wd["pq"])
        if sp["im"]:
            feats["ims"] = wd["f"]["ims"]
        wd["cache"]["fmap"] = (RI if sp["im"] else R).build_feature_map(W.settings_of(wd["name"]), sp["charge"], feats)
        wd["cache"]["ref_spectra"] = (T.ref_spectra_im if sp["im"] else T.ref_spectra)(wd["batches"])
    spectra = wd["cache"]["ref_spectra"]
    if subset is not None:
        spectra = [spectra[i] for i in subset]
    return (RI if sp["im"] else R).trace(wd["cache"]["fmap"], spectra, wd["alignments"], wd["n_files"], sp["combine"], T.isotopes_of(wd["db"]))


def assert_same_grids(got, want, what):
    assert sorted(got) == sorted(want), f"{what}: grid keys"
    for k in sorted(got):
        a, b = got[k].view(np.uint64), np.ascontiguousarray(want[k]["matrix"]).view(np.uint64)
        if not np.array_equal(a, b):
            row, col = (int(x[0]) for x in np.nonzero(a != b))
            raise AssertionError(f"{what}: grid {k} row {row} bin {col}: {got[k][row, col]!r} != {want[k]['matrix'][row, col]!r}")


@pytest.mark.parametrize("name", W.NAMES)
def test_census(name):
    wd = W.world(name)
    figures = W.census(wd)
    print(name, figures)
    assert figures["windows"] == W.WINDOWS[name] and figures["pages"] == W.PAGES[name]
    # the pruned matcher (the one tests/test_gpu_lfq_trace.py uses) finds the exhaustive one's matches, in its order
    (grids, n, m), (grids_p, n_p, m_p) = W.brute(wd), W.brute(wd, prune=True)
    assert n == n_p and sorted(m) == sorted(m_p)
    for k in m:
        assert m[k].dtype == m_p[k].dtype and np.array_equal(m[k], m_p[k]), k
    assert sorted(grids) == sorted(grids_p) and all(np.array_equal(grids[k].view(np.uint64), grids_p[k].view(np.uint64)) for k in grids)


@pytest.mark.parametrize("name", W.NAMES)
def test_pages_are_the_restatements(name):
    wd = W.world(name)
    _restatement(wd, subset=[])
    fmap, w = wd["cache"]["fmap"], wd["windows"]
    index = {k: i for i, k in enumerate(zip(w["peptide"].tolist(), w["charge"].tolist(), w["isotope"].tolist(), w["decoy"].tolist()))}
    at = np.array([index[(e["peptide"], e["charge"], e["isotope"], bool(e["decoy"]))] for e in fmap["ranges"]])
    assert len(at) == len(w["rt"]) == len(set(at.tolist()))
    assert np.array_equal(wd["page"][at], np.arange(len(at)) // R.BIN_SIZE)
    assert [float(x) for x in fmap["min_rts"]] == [float(x) for x in wd["min_rts"]]
    for key in ("rt", "mass_lo", "mass_hi") + (("mobility_lo", "mobility_hi") if wd["spec"]["im"] else ()):
        assert np.array_equal(np.array([e[key] for e in fmap["ranges"]], np.float32).view(np.uint32), w[key][at].view(np.uint32)), key


@pytest.mark.parametrize("name", W.NAMES)
def test_brute_force_equals_restatement(name):
    wd = W.world(name)
    subset = None
    if name not in ("p1", "p2"):
        seam = W.seam_spectra(wd)
        assert len(seam) >= W.PAGES[name] - 2 + W.PAGES[name] - 2
        rest = [i for i, s in enumerate(wd["given"]) if i not in seam]
        subset = sorted(seam + [i for i in rest if wd["given"][i].kind in ("last-slot", "low")] + rest[::2] + rest[1::4])
    got, n, _ = W.brute(wd, subset)
    assert n > 1000
    assert_same_grids(got, _restatement(wd, subset), name)


@pytest.fixture(scope="module")
def db():
    return T.database()


def _existing(world, charge, ppm, im, combine, pct=1.0):
    f = world["f"]
    w = B.build_windows(f["peptide_idx"], f["label"], f["calcmass"], world["art"], world["pq"], charge, ppm,
                        ims=f["ims"] if im else None, mobility_pct=pct)
    B.require_layout_free(w)
    return B.trace(w, B.read_spectra(world["batches"]), world["alignments"], len(world["alignments"]), combine)


def test_existing_worlds(db):
    run = T.run_world(db)
    got, n, _ = _existing(run, (2, 4), 5.0, False, True)
    fmap = R.build_feature_map(R.default_settings(), (2, 4), T.ref_feats(run["f"], run["art"], run["pq"]))
    assert n > 1000
    assert_same_grids(got, R.trace(fmap, run["spectra"], run["alignments"], 3, True, T.isotopes_of(db)), "run_world")
    refused = []
    for i in range(T.N_WORLDS):
        n_files, charge, combine, ppm, im, settings = T.param_settings(i)
        world = T.param_world(db, i)
        try:
            got, n, _ = _existing(world, charge, ppm, im, combine, settings["mobility_pct_tolerance"])
        except B.NotLayoutFree as e:
            print(f"param_world({i}), {ppm} ppm, charges {charge}: {e}")
            refused.append(i)
            continue
        assert n > 100
        assert_same_grids(got, world["grids"], f"param_world({i})")
    print("refused:", refused)
    assert tuple(refused) == REFUSED == tuple(i for i in range(T.N_WORLDS) if T.param_settings(i)[3] == 50.0)
