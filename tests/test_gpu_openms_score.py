"""OpenMSHyperScore on the device, held BY BITS to numbers that come from the CPU alone, on the aimed worlds of
tests/openms_worlds.py: the summed intensity of every spectrum is a chosen f32 bit pattern (the hard arguments of the f32 ln_1p, the
six where the correctly rounded double rounds to the wrong float, thousands where the platform's log1pf is an ulp off, both sides
of every binade edge from 2^-30 to 2^127, FLT_MAX, +-0, +inf, an overflowing b + y sum, a log-uniform fill), and

    hyperscore = (double)ref_ln1pf(si) + lnfact(matched_b) + lnfact(matched_y)       (255.0 where that is not finite)

with ref_ln1pf libquadmath's log1pq rounded once and lnfact over the oracle's correctly rounded ln.  The oracle in its correctly
rounded mode is held to the same numbers without a device (test_the_oracle_computes_the_expected_numbers).

Every kernel that evaluates the score is reached, and each test says how it knows:
  rescore_kernel, first pass (the logarithm's fast phase only)   sage_hip_debug_rescore_instance: no ACC, no BIG bit; n_retry == 0
  the retry pass (both phases)                                   n_retry == every spectrum: hundreds of equal hyperscores at rank 2
      narrow_kernel (the retry pass of a narrow search is this   ... n_wide == 0
      kernel with the exact settings; as a first pass it exists
      in experiment builds only)
      rescore_kernel's ACC instance behind the large-window      ... SAGE_HIP_WCAP=64: n_wide > 0
      kernels
  rescore_big_kernel                                             report_psms = 33: instance BIG
  candidates_kernel                                              sage_hip_score_candidates_resident's own records
  score_batch, host to host                                      Scorer.score

A summed intensity that is NaN or negative cannot be produced through the kernels (select_most_intense_peak takes `intensity >= 0`
only): such peaks give no PSM on either side, and cr_log1pf's values there are held exhaustively by tests/test_ln1pf_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import openms_worlds as W
import test_ln1pf_cpu as LN
from parity_utils import assert_features_equal
from sage_amd import _lib as L
from sage_amd.api import Scorer

INST_ACC, INST_BIG, INST_NONE = 8, 32, 0xFFFFFFFF
ENV = ("SAGE_HIP_WCAP", "SAGE_HIP_EXACT", "SAGE_HIP_DEBUG_FLAGS", "SAGE_HIP_PHASE_CLOCKS", "SAGE_HIP_RESCORE_GENERAL",
       "SAGE_HIP_ONE_LAUNCH", "SAGE_HIP_NARROW", "SAGE_HIP_NO_FAST_TIES", "SAGE_HIP_NO_SCHED")
u64 = np.uint64


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(u64), np.ascontiguousarray(b, np.float64).view(u64))


# ---- the cases: inputs and expected numbers, once per session, CPU only --------------------------------------------------------------
_cases, _oracle = {}, {}


def case(name):
    if name in _cases:
        return _cases[name]
    w, c = W.world(), {}
    if name == "singles":
        groups = W.single_arguments()
        c["groups"] = groups
        bits = np.concatenate(list(groups.values()))
        assert len(bits) == W.MAX_SPECTRA
        c["batch"], c["pep"], is_b = W.singles(w, bits)
        c["si"] = np.where(bits == 0x80000000, 0, bits).astype(np.uint32)   # 0.0f + -0.0f == +0.0f
        c["matched"] = (is_b.astype(int), 1 - is_b.astype(int))
        c["params"] = W.single_params()
    elif name == "sums":
        args = np.concatenate([np.array(LN.HARD_POSITIVE, np.uint32), W.libm_wrong_arguments(40)])
        c["batch"], c["pep"], c["si"] = W.sums(w, args)
        n = len(c["si"])
        c["matched"] = (np.ones(n, int), np.ones(n, int))
        c["params"] = W.single_params()
    elif name == "ties":
        bits = W.tie_arguments()
        c["batch"], c["pep"], is_b = W.ties(w, bits)
        c["si"] = bits
        c["matched"] = (1 + is_b.astype(int), 1 - is_b.astype(int))
        c["params"] = W.pair_params()
    elif name == "unmatched":
        c["batch"], c["pep"], _ = W.singles(w, W.UNMATCHED)
        c["params"] = W.single_params()
    else:
        assert name == "pairs"
        c["batch"], c["rows"] = W.ranking_pairs(w)
        c["params"] = W.pair_params()
    if "si" in c:
        h = np.zeros(len(c["si"]))
        for mb, my in sorted(set(zip(*c["matched"]))):
            sel = (c["matched"][0] == mb) & (c["matched"][1] == my)
            h[sel] = W.expected_hyperscore(c["si"][sel], int(mb), int(my))
        c["hyperscore"] = h
    _cases[name] = c
    return c


def oracle_records(name, **kw):
    """the oracle's records (correctly rounded mode) for a case under its parameters with `kw` changed"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _oracle:
        c = case(name)
        p = W.single_params(**dict(c["params"].__dict__, **kw))
        of, oc, _, _ = W.world().oracle.score(p, c["batch"])
        _oracle[key] = (p, of, oc)
    return _oracle[key]


def hold_first_rank(c, feats, counts, context):
    """rank 1 of every spectrum: the home peptide, its matched peaks, its hyperscore by bits"""
    assert (counts >= 1).all(), f"{context}: {int((counts == 0).sum())} spectra without a PSM"
    top = feats[:, 0]
    assert np.array_equal(top["peptide_idx"], c["pep"]), context
    assert np.array_equal(top["matched_peaks"], c["matched"][0] + c["matched"][1]), context
    assert np.array_equal(top["ms2_intensity"].view(np.uint32), c["si"]), f"{context}: the summed intensity is not the aimed one"
    got, want = top["hyperscore"], c["hyperscore"]
    if not same_bits(got, want):
        bad = np.flatnonzero(got.view(u64) != want.view(u64))
        raise AssertionError(f"{context}: hyperscore differs on {len(bad)} spectra, first summed intensities "
                             f"{[hex(v) for v in c['si'][bad[:6]]]}: got {got[bad[:6]]!r}, expected {want[bad[:6]]!r}")


def hold_pairs(c, feats, counts, context):
    rows = c["rows"]
    assert (counts == 2).all(), context
    on_p, on_q = (np.array([r[k] for r in rows], np.uint32) for k in (2, 3))
    hp, hq = W.expected_hyperscore(on_p, 1, 0), W.expected_hyperscore(on_q, 1, 0)
    n_same = n_diff = 0
    for i, (p, q, _, _, is_same) in enumerate(rows):
        first, second = feats[i, 0], feats[i, 1]
        assert {int(first["peptide_idx"]), int(second["peptide_idx"])} == {p, q}, f"{context}: spectrum {i}"
        if is_same:
            assert hp[i] == hq[i]
            if i % 2:   # the same two candidates with the intensities swapped: the tie order does not follow the intensity
                assert first["peptide_idx"] == feats[i - 1, 0]["peptide_idx"], f"{context}: spectrum {i}: a tie was ordered by the intensity"
            n_same += 1
        else:
            assert hp[i] != hq[i]
            assert int(first["peptide_idx"]) == (p if hp[i] > hq[i] else q), f"{context}: spectrum {i}: the order does not follow the score"
            n_diff += 1
        h1, h2 = max(hp[i], hq[i]), min(hp[i], hq[i])
        want = np.array([h1, h1 - h2, h1 - h1, h2, h2 - 0.0, h1 - h2])
        got = np.array([first["hyperscore"], first["delta_next"], first["delta_best"], second["hyperscore"], second["delta_next"],
                        second["delta_best"]])
        assert same_bits(got, want), f"{context}: spectrum {i}: hyperscore / delta_next / delta_best {got!r}, expected {want!r}"
    assert n_same >= 100 and n_diff >= 100, (n_same, n_diff)


def hold_ties(c, feats, counts, context):
    hold_first_rank(c, feats, counts, context)
    assert (counts == feats.shape[1]).all(), context   # (report_psms of the hundreds of candidates)
    h2 = W.expected_hyperscore(np.array([0x3F800000], np.uint32), 1, 0)[0]   # intensity 1 on b1 alone
    h1 = c["hyperscore"]
    assert (h1 > h2).all()
    n = len(h1)
    assert same_bits(feats[:, 1]["hyperscore"], np.full(n, h2)) and same_bits(feats[:, 0]["delta_next"], h1 - h2), context
    assert same_bits(feats[:, 1]["delta_best"], h1 - h2) and same_bits(feats[:, 1]["delta_next"], np.zeros(n)), context


HOLD = {"singles": hold_first_rank, "sums": hold_first_rank, "ties": hold_ties, "pairs": hold_pairs}


# ---- without a device: the oracle against the expected numbers ---------------------------------------------------------------------
def test_the_worlds_hold_what_they_promise():
    w, c = W.world(), case("singles")
    g = c["groups"]
    assert w.db.n_peptides == W.N_PEPTIDES and len(w.homes) >= 60 and c["batch"].n == W.MAX_SPECTRA
    assert set(LN.DOUBLE_ROUNDING) <= set(int(v) for v in g["hard"]) and len(g["hard"]) == 45
    wrong = g["libm wrong"]
    assert len(wrong) >= 2000 and np.all(LN.libm_log1pf(wrong) != LN.ref_ln1pf(wrong)), "thousands of arguments the platform's log1pf gets wrong"
    assert len(g["binade edges"]) == 3 * 158 + 1 and 255.0 in c["hyperscore"] and (c["hyperscore"] != 255.0).sum() >= W.MAX_SPECTRA - 2
    assert case("sums")["si"][-1] == W.INF and case("sums")["hyperscore"][-1] == 255.0 and len(case("sums")["si"]) >= 100
    assert len(case("ties")["si"]) >= 150


@pytest.mark.parametrize("name", ["singles", "sums", "ties", "pairs"])
def test_the_oracle_computes_the_expected_numbers(name):
    c = case(name)
    _, of, oc = oracle_records(name)
    HOLD[name](c, of, oc, f"oracle, {name}")


def test_peaks_that_are_never_matched_give_no_psm_in_the_oracle():
    _, of, oc = oracle_records("unmatched")
    assert (oc == 0).all(), "NaN and negative intensities are never the most intense peak (spectrum.rs:149-153)"


# ---- on the device --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def dev(gpu_required, monkeypatch):
    from test_gpu_index_tables import create
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    d = create(monkeypatch, {}, W.world().db)
    yield d
    d.close()


def run(dev, name, **kw):
    """the case on a fresh scorer: (scorer, device batch, records, counts, the step's timing, the rescoring instance it launched);
    the records are held to the oracle's, every field, and to the expected numbers"""
    c = case(name)
    p, of, oc = oracle_records(name, **kw)
    scorer = Scorer(dev, p)
    dbatch = scorer.upload(c["batch"])
    gf, gc = scorer.score_resident(dbatch)
    gf, gc = gf.copy(), gc.copy()
    t = scorer.last_timing()
    inst = np.zeros(1, np.uint32)
    L.check(L.load().sage_hip_debug_rescore_instance(scorer._h, L.as_ptr(inst, C.c_uint32)))
    context = f"{name} {kw}"
    assert_features_equal(gf, gc, of, oc, context)
    HOLD[name](c, gf, gc, context)
    return scorer, dbatch, gf, gc, t, int(inst[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["singles", "sums", "pairs"])
def test_first_pass_of_rescore_kernel(dev, name):
    """The production route: prelim_kernel, then the rescore_kernel instance that carries the logarithm's fast phase only.  No
    spectrum of the singles and the sums went to the retry pass, so every record is that instance's.  Of the pairs, at most the
    spectra whose two hyperscores are EQUAL did (measured: all 300 of them, through narrow_kernel — their tie order is held there);
    the 300 whose order follows the score were ranked by the first pass."""
    scorer, dbatch, gf, gc, t, inst = run(dev, name)
    assert inst != INST_NONE and not inst & (INST_ACC | INST_BIG), f"instance {inst:#x}"
    equal = sum(r[4] for r in case(name)["rows"]) if name == "pairs" else 0
    assert t["n_retry"] <= equal and t["n_wide"] == 0, t
    print(f"{name}: {t['n_retry']} of {case(name)['batch'].n} spectra took the retry pass")
    scorer.close()


@pytest.mark.gpu
def test_unmatched_peaks_give_no_psm(dev):
    c = case("unmatched")
    scorer = Scorer(dev, c["params"])
    gf, gc = scorer.score_resident(scorer.upload(c["batch"]))
    assert (gc == 0).all()
    scorer.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wcap", [None, "64"])
def test_retry_pass(dev, monkeypatch, wcap):
    """Every spectrum's second rank is one of hundreds of equal hyperscores in a list the k-select had to trim: all of them are sent
    to the exact retry pass (n_retry), whose kernels carry both phases of the logarithm — narrow_kernel with the exact settings, or,
    with SAGE_HIP_WCAP=64, the large-window kernels and rescore_kernel's ACC instance behind them (n_wide)."""
    if wcap:
        monkeypatch.setenv("SAGE_HIP_WCAP", wcap)
    scorer, dbatch, gf, gc, t, inst = run(dev, "ties")
    assert t["n_retry"] == case("ties")["batch"].n, t
    assert (t["n_wide"] > 0) == (wcap is not None), t
    scorer.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["singles", "ties"])
def test_rescore_big_kernel(dev, name):
    """report_psms beyond 32 takes rescore_big_kernel"""
    scorer, dbatch, gf, gc, t, inst = run(dev, name, report_psms=33)
    assert inst == INST_BIG, f"instance {inst:#x}"
    scorer.close()


@pytest.mark.gpu
def test_candidates_kernel_and_score_batch(dev):
    """sage_hip_score_candidates_resident scores the home peptide on each spectrum once more (candidates_kernel); Scorer.score is
    the host-to-host entry point, sage_hip_score_batch"""
    for name in ("singles", "sums"):
        c = case(name)
        scorer, dbatch, gf, gc, t, inst = run(dev, name)
        n = c["batch"].n
        out = scorer.score_candidates(dbatch, gf, gc, np.arange(n + 1, dtype=np.uint64), c["pep"])
        assert np.array_equal(out["matched_b"], c["matched"][0]) and np.array_equal(out["matched_y"], c["matched"][1]), name
        with np.errstate(all="ignore"):
            assert np.array_equal((out["summed_b"] + out["summed_y"]).view(np.uint32), c["si"]), name
        assert same_bits(out["hyperscore"], c["hyperscore"]), f"{name}: candidates_kernel"
        gf2, gc2 = scorer.score(c["batch"])
        HOLD[name](c, gf2, gc2, f"{name}, score_batch")
        assert gf2.tobytes() == gf.tobytes() and np.array_equal(gc2, gc), f"{name}: score_batch differs from the resident step"
        scorer.close()
