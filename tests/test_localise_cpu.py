"""Site localisation without a device: the plain restatement (tests/localise_reference.py) against a case worked
by hand, and the library's host arithmetic (sage_hip_ascore_from_counts) against the restatement on random integer counts.
(sage_hip_localise_resident needs a scorer and a resident batch, that is a device: tests/test_gpu_localise.py.)"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import localise_reference as LR
import second_reading as SR
from sage_amd import _lib as L
from sage_amd.api import ScorerParams, ascore_from_counts

f32 = np.float32


def _hand_world():
    """AASATAK with one phospho: placement A on the serine (residue 3), placement B on the threonine (residue 5); b and y ions,
    precursor charge 2 (one fragment charge), 10 ppm"""
    seq = b"AASATAK"
    ph = f32(79.9663)
    mods = {0: [0, 0, ph, 0, 0, 0, 0], 1: [0, 0, 0, 0, ph, 0, 0]}
    mono = []
    for m in mods.values():
        total = f32(0)
        for r, x in zip(seq, m):
            total = total + SR.MONO[r - 65] + f32(x)
        mono.append(total + SR.H2O)
    arrays = dict(pep_mono=np.array(mono, np.float32), seq_off=[0, 7, 14], seq=np.frombuffer(seq * 2, np.uint8),
                  mods=np.array(mods[0] + mods[1], np.float32), nterm=np.array([np.nan, np.nan], np.float32), decoy=[0, 0], missed=[0, 0])
    return SR.SecondScorer(SR.Peptides(arrays), [SR.B, SR.Y], 2, ScorerParams(report_psms=1))


def test_a_case_worked_by_hand():
    """The spectrum holds placement A's twelve ions; the k-th peak in mass order has intensity 100 + k, so inside a 100-window the
    heavier peak outranks the lighter one:

        window 0: 71.04 (b1)                                       rank 1
        window 1: 142.07 (b2), 146.11 (y6)                         ranks 2, 1
        window 2: 217.14 (y5)                                      rank 1
        window 3: 309.07 (b3), 318.19 (y4), 380.11 (b4), 389.23 (y3)   ranks 4, 3, 2, 1
        window 4: 481.16 (b5)                                      rank 1
        window 5: 552.19 (b6), 556.23 (y2)                         ranks 2, 1
        window 6: 627.26 (y1)                                      rank 1

    A's items b1..b6, y1..y6 have min-ranks 1 2 4 2 1 2 | 1 1 1 3 1 1.  B shares b1, b2, b5, b6, y1, y2 and — within 10 ppm,
    their f32 values differ in the last bits — y5, y6; its b3, b4, y3, y4 (229.11, 300.14, 469.19, 398.16) meet no peak:
    1 2 - - 1 2 | 1 1 - - 1 1.  Site-determining by bit pattern: b3, b4, y3, y4 and the two rounded differently, y5, y6."""
    sr = _hand_world()
    ions_a = np.array([ion for ion, _ in LR.items(sr, 0, 2)], np.float32)
    assert len(ions_a) == 12
    masses = np.sort(ions_a)
    intens = (f32(100.0) + np.arange(12, dtype=np.float32)).astype(np.float32)
    assert [round(float(m), 2) for m in masses] == [71.04, 142.07, 146.11, 217.14, 309.07, 318.19, 380.11, 389.23, 481.16, 552.19,
                                                    556.23, 627.26]
    assert list(LR.depth_ranks(masses, intens)) == [1, 2, 1, 1, 4, 3, 2, 1, 1, 2, 1, 1]
    ranks = LR.depth_ranks(masses, intens)
    assert LR.item_min_ranks(sr, masses, ranks, 0, 2) == [1, 2, 4, 2, 1, 2, 1, 1, 1, 3, 1, 1]
    assert LR.item_min_ranks(sr, masses, ranks, 1, 2) == [1, 2, 255, 255, 1, 2, 1, 1, 255, 255, 1, 1]
    # B first in the list: the best placement is found by its score, not by its position
    got = LR.localise(sr, masses, intens, [1, 0], [2, 2])
    assert got["counts"] == [([6, 8, 8, 8, 8, 8, 8, 8, 8, 8], 12), ([7, 10, 11, 12, 12, 12, 12, 12, 12, 12], 12)]
    assert (got["best"], got["second"]) == (1, 0) and got["best_score"] > got["second_score"] > 0.0
    assert got["n_site_items"] == 6
    assert got["a"] == [3, 4, 5, 6, 6, 6, 6, 6, 6, 6]
    assert got["b"] == [2, 2, 2, 2, 2, 2, 2, 2, 2, 2]
    assert got["depth"] == 4  # a - b = 1, 2, 3, 4, 4, ...: the first depth with the largest difference
    # S(6, 6, 4) = -10 log10(0.04 ^ 6); S(2, 6, 4) = -10 log10(1 - 0.96 ^ 6 - 6 * 0.04 * 0.96 ^ 5)
    want = -60.0 * math.log10(0.04) + 10.0 * math.log10(1.0 - 0.96 ** 6 - 6 * 0.04 * 0.96 ** 5)
    assert got["ascore"] > 0.0 and abs(got["ascore"] - want) < 1e-9 * want
    # one candidate: no second, no Ascore
    alone = LR.localise(sr, masses, intens, [0], [2])
    assert (alone["best"], alone["second"], alone["n_site_items"], alone["depth"]) == (0, LR.NONE, 0, 0) and math.isnan(alone["ascore"])
    # equal scores: the smaller position is the best one
    twice = LR.localise(sr, masses, intens, [0, 0], [2, 2])
    assert (twice["best"], twice["second"], twice["n_site_items"], twice["depth"], twice["ascore"]) == (0, 1, 0, 1, 0.0)


def test_the_depth_score_in_closed_form():
    assert LR.depth_score(0, 50, 3) == 0.0 and LR.depth_score(0, 0, 3) == 0.0
    assert abs(LR.depth_score(1, 1, 10) - 10.0) < 1e-12                       # P = 0.1
    assert abs(LR.depth_score(1, 2, 5) + 10.0 * math.log10(1 - 0.95 ** 2)) < 1e-12
    assert abs(LR.depth_score(600, 600, 1) - 12000.0) < 1e-8                  # 0.01 ^ 600 underflows as a product
    assert abs(LR.peptide_score([1] * 10, 1) - sum(w * -10.0 * math.log10(d / 100.0) for d, w in zip(range(1, 11), LR.WEIGHTS)) / 7.0) < 1e-12


def _both(n, N):
    got = ascore_from_counts(n=n, n_items=N)
    want = [LR.depth_score(int(n[d - 1]), N, d) for d in range(1, 11)]
    return got, want


def test_host_arithmetic_in_closed_form():
    """what does not depend on lgamma's last bits: the exact zeros, single-term sums, the case whose plain product underflows"""
    assert 0.01 ** 600 == 0.0
    got = ascore_from_counts(n=np.full(10, 600, np.uint16), n_items=600)["depth_scores"]
    for d in range(1, 11):  # P = (d / 100) ^ 600
        assert math.isfinite(got[d - 1]) and abs(got[d - 1] + 6000.0 * math.log10(d / 100.0)) < 1e-9 * 12000.0
    assert not ascore_from_counts(n=np.zeros(10, np.uint16), n_items=600)["depth_scores"].any()
    assert not ascore_from_counts(n=np.zeros(10, np.uint16), n_items=0)["depth_scores"].any()
    assert ascore_from_counts(n=np.zeros(10, np.uint16), n_items=0)["peptide_score"] == 0.0
    one = ascore_from_counts(n=np.ones(10, np.uint16), n_items=1)
    assert all(abs(one["depth_scores"][d - 1] + 10.0 * math.log10(d / 100.0)) < 1e-12 for d in range(1, 11))


def test_host_arithmetic_equals_the_restatement_on_random_counts():
    """1e-12 relative to max(|S|, 1), the tolerance tests/test_gpu_isomers.py grants an f64.  A small S is a difference of
    log-gammas of up to 3 200 whose last bit weighs 4.5e-13, so two log-gamma functions that differ in their last bits do not
    hold it: the library evaluates the Lanczos approximation math.lgamma evaluates (localise_math.h: lgamma_lanczos), not the C
    library's lgamma, and log and exp are the C library's on both sides."""
    rng = np.random.default_rng(11)
    cases = [(np.zeros(10, np.uint16), 0), (np.zeros(10, np.uint16), 600), (np.full(10, 600, np.uint16), 600),
             (np.full(10, 1, np.uint16), 1), (np.arange(1, 11).astype(np.uint16), 10)]
    for _ in range(300):
        N = int(rng.integers(0, 601))
        cases.append((rng.integers(0, N + 1, 10).astype(np.uint16), N))
    worst, missed = 0.0, []
    for n, N in cases:
        got, want = _both(n, N)
        for d in range(10):
            g, w = float(got["depth_scores"][d]), want[d]
            assert math.isfinite(g), (n, N, d + 1)
            worst = max(worst, abs(g - w) / max(abs(w), 1.0))
            if not LR.close(g, w):
                missed.append(f"S({int(n[d])}, {N}, {d + 1}): library {g!r} vs restatement {w!r}")
            if n[d] == 0 or N == 0:
                assert g == 0.0
        if not LR.close(got["peptide_score"], LR.peptide_score([int(x) for x in n], N)):
            missed.append(f"peptide score of {list(n)} of {N}")
    print(f"largest gap between the library's and the restatement's depth scores, relative to max(|S|, 1): {worst:.3e}; "
          f"{len(missed)} values beyond 1e-12")
    assert not missed, missed[:5]


def test_ascore_and_depth_equal_the_restatement_on_random_counts():
    rng = np.random.default_rng(12)
    for trial in range(300):
        Ns = int(rng.integers(0, 200)) if trial else 0
        a = np.sort(rng.integers(0, Ns + 1, 10)).astype(np.uint16)
        b = np.sort(rng.integers(0, Ns + 1, 10)).astype(np.uint16)
        if trial % 7 == 1:
            b = a.copy()  # every difference zero: depth 1
        got = ascore_from_counts(a=a, b=b, n_site_items=Ns)
        depth, score = LR.ascore([int(x) for x in a], [int(x) for x in b], Ns)
        assert got["depth"] == depth and LR.close(got["ascore"], score), (a, b, Ns, got, depth, score)
    assert ascore_from_counts(a=[0] * 10, b=[0] * 10, n_site_items=0) == dict(depth=1, ascore=0.0)


def test_host_arithmetic_stand_alone_under_sanitizers(tmp_path):
    """localise_math.h as a program of its own (tests/hostemu/localise_math_emu.cpp), with AddressSanitizer and
    UndefinedBehaviorSanitizer: the depth-score cache starts again past 2^23 values and hands out the same bits before, after and
    from a fresh cache; ascore_of without site-determining items and with a tie between depths"""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "localise_math_emu_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(here, "hostemu", "localise_math_emu.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "localise_math_emu ok" in r.stdout, r.stdout + r.stderr


def test_counts_above_their_total_are_refused():
    with pytest.raises(L.SageHipError, match="status 1"):
        ascore_from_counts(n=[0] * 9 + [5], n_items=4)
    with pytest.raises(L.SageHipError, match="status 1"):
        ascore_from_counts(a=[0] * 10, b=[3] * 10, n_site_items=2)


def test_abi_version_and_exported_symbols():
    lib = L.load()
    assert lib.sage_hip_abi_version() == 6
    new = ["sage_hip_localise_resident", "sage_hip_ascore_from_counts", "sage_hip_last_localise_timing"]
    assert all(s in L.EXPORTED_SYMBOLS for s in new)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sage_hip.h")).read()
    for s in new:
        assert f" T {s}\n" in dynamic, f"{s} is not exported"
        assert f" {s}(" in header, f"{s} is not declared in sage_hip.h"
    assert L.DEPTH_COUNTS_DTYPE.itemsize == 11 * 2 + 2 == 24
    assert L.LOCALISATION_DTYPE.itemsize == 3 * C.sizeof(C.c_double) + 3 * 4 + 20 * 2 + 4 == 80
    assert L.LOCALISATION_DTYPE.fields["depth"][1] == 76 and L.LOCALISATION_DTYPE.fields["a"][1] == 36
