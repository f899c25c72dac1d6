"""The world of tests/handle_sequences.py held to what tests/test_gpu_handle_sequences.py rests on — no device needed."""
import dataclasses

import numpy as np
import pytest

import handle_sequences as H
from parity_utils import assert_features_equal
from sage_amd.cli import isomer_candidates


@pytest.fixture(scope="module")
def w():
    return H.world()


def test_quiet_windows_hold_fewer_peptides_than_a_trim_keeps(w):
    """Q, Q2 (first configuration) and N (second): no preliminary list can be trimmed, so nothing can be retried.  R and W are
    the opposite: most of their windows hold more."""
    for cfg, name in (("main", "Q"), ("main", "Q2"), ("main", "BIGQ"), ("second", "N")):
        c = w.window_counts(cfg, name)
        assert c.min() >= 1 and c.max() < H.trim_k(H.CONFIGS[cfg]), (cfg, name, int(c.max()))
    assert np.mean(w.window_counts("main", "R") > H.trim_k(H.CONFIGS["main"])) > 0.8
    assert np.mean(w.window_counts("second", "W") > H.trim_k(H.CONFIGS["second"])) > 0.9
    assert not set(w.index["Q"]) & set(w.index["Q2"])


def test_the_heavy_block_lies_above_every_twin_peptide(w):
    assert w.heavy.sum() >= 80
    assert w.host.pep_mono[w.heavy].min() > w.host.pep_mono[~w.heavy].max() + 2 * 200.0  # (apart by more than the widest window)
    for i in np.flatnonzero(w.heavy)[:20]:
        assert not set(w.host.sequence(int(i))) & set("ILM")


def test_big_is_separated_by_mass_and_a_third_at_most_is_retry_rich(w):
    """Every R spectrum's neutral precursor mass below every Q spectrum's: in the launch schedule (sorted by that mass) the R
    spectra of BIG are one contiguous run at one end, shorter than a third — of two or three contiguous parts at least one holds
    none of them and at least one holds some."""
    r, q = H.neutral_mass(w.batch("R")), H.neutral_mass(w.batch("Q"))
    assert r.max() < q.min()
    big, from_r = w.index["BIG"], w.index["BIG"] < H.N_TWIN_SPECTRA
    assert len(big) == len(w.index["BIGQ"]) == H.N_BIG and 0 < from_r.sum() <= H.N_BIG // 3
    assert set(big[from_r]) == set(w.index["R"]) and set(big[~from_r]) == set(w.index["Q"]) == set(w.index["BIGQ"])
    assert (w.batch("BIG").precursor_charge > 0).all() and (w.batch("R").precursor_charge > 0).all()
    order = np.argsort(H.neutral_mass(w.batch("BIG")), kind="stable")
    for ways in (2, 3):
        per_part = [int(from_r[order[H.N_BIG * k // ways: H.N_BIG * (k + 1) // ways]].sum()) for k in range(ways)]
        assert min(per_part) == 0 and max(per_part) > 0, per_part
    s65 = w.index["S65"]
    assert len(s65) == 65 and 20 < (s65 < H.N_TWIN_SPECTRA).sum() < 45
    assert len(w.index["S1"]) == 1 and w.index["S1"][0] in w.index["R"] and len(w.index["E"]) == 0
    for name, idx in w.index.items():
        assert name in ("BIG", "BIGQ") or len(idx) <= 1000


def test_big_under_the_second_configuration_is_wide_in_its_twin_spectra_only(w):
    """What test_gpu_handle_sequences.test_a_wrong_guess_in_parts_is_repeated_as_one rests on: under ±200 Da the twin spectra
    of BIG have windows beyond the narrow kernel's capacity (DevScorer::wcap, 1024 candidate slots) — the step must be repeated
    with the large-window kernels — and the heavy ones, three quarters of the batch and the whole of one part, have none."""
    wcap = 1024
    c = w.window_counts("second", "BIG")
    from_r = w.index["BIG"] < H.N_TWIN_SPECTRA
    print(f"twin windows {int(c[from_r].min())} .. {int(c[from_r].max())}, heavy windows {int(c[~from_r].min())} .. {int(c[~from_r].max())}")
    assert c[from_r].max() > wcap and np.mean(c[from_r] > wcap) > 0.5
    assert c[~from_r].max() < H.trim_k(H.CONFIGS["second"])
    assert H.N_BIG >= 2 * 8192 and "BIG" in H.BATCHES_OF["second"]
    # the oracle of BIG under the second configuration is a gather over the same unique spectra as under the first
    used = w.oracle_unique("second")[2]
    assert set(w.index["BIG"]) <= set(used)


def test_the_oracle_reports_on_r_and_its_last_rank_is_tied(w):
    """At least 2 n / 3 PSMs on R, and for at least 50 of its spectra the last reported hyperscore equals that of another
    candidate in the window — the tie the retry pass exists for.  Read from the oracle with report_psms one higher: rank 2 against
    rank 3, and against rank 1.  In this world the twins tie in pairs (a peptide and its mirror; their decoys are each other's
    mirrors too), so nearly every tie is between ranks 1 and 2: 5 spectra tie at ranks 2 and 3, 238 at ranks 1 and 2."""
    of, oc = w.oracle("main", "R")
    n = len(oc)
    assert int(oc.sum()) >= 2 * n // 3
    params = H.CONFIGS["main"]
    more = dataclasses.replace(params, report_psms=params.report_psms + 1)
    f3, c3, _, _ = w.orc.score(more, w.batch("R"))
    h = f3["hyperscore"]
    last = params.report_psms - 1
    behind = (c3 == more.report_psms) & (h[:, last] == h[:, last + 1])  # ranks 2 and 3
    ahead = (c3 >= params.report_psms) & (h[:, last] == h[:, last - 1])  # ranks 1 and 2: a peptide and its I / L twin
    tied = behind | ahead
    print(f"last reported hyperscore tied with the rank behind it: {int(behind.sum())} spectra, with the rank ahead: {int(ahead.sum())}")
    assert int(tied.sum()) >= 50, (int(behind.sum()), int(ahead.sum()))
    assert tied[w.index["S1"][0]], "S1 is a spectrum of R with the tie"
    assert (tied[w.index["S65"][w.index["S65"] < H.N_TWIN_SPECTRA]]).sum() >= 5
    # the candidate lists of the command line's calls are not empty on R
    off, _ = isomer_candidates(w.groups, of, oc)
    assert int(off[-1]) >= 20
    oq, cq = w.oracle("main", "Q")
    assert int(cq.sum()) >= 200 and int(w.oracle("second", "N")[1].sum()) >= 150 and int(w.oracle("second", "W")[1].sum()) >= 150


def test_expansion_by_index_is_the_oracle_on_the_expanded_batch(w):
    lo = 11111
    idx = np.arange(lo, lo + 2048)
    of, oc = w.oracle("main", "BIG")
    f, c, _, _ = w.orc.score(H.CONFIGS["main"], w.batch("BIG").subset(idx))
    want = of[idx].copy()
    want["spec_index"] -= lo
    assert assert_features_equal(want, oc[idx], f, c, "BIG[11111:13159]") > 2048
    assert c.tobytes() == oc[idx].tobytes()
    mask = np.arange(f.shape[1])[None, :] < c[:, None]
    assert want[mask].tobytes() == f[mask].tobytes()
    f, c, _, _ = w.orc.score(H.CONFIGS["second"], w.batch("W"))
    assert_features_equal(*w.oracle("second", "W"), f, c, "W")


def test_drawn_sequences_are_reproducible_and_cover_the_alphabet(w):
    seqs = [H.draw_sequence(seed) for seed in range(12)]
    assert seqs == [H.draw_sequence(seed) for seed in range(12)]
    kinds = {k for s in seqs for k, _ in s}
    assert kinds >= {"pinned", "pageable", "stream", "reupload", "annotate", "candidates", "hits", "quick0", "quick1", "timing", "clone"}
    for s in seqs:
        assert len(s) == 14 and sum(b in ("BIG", "BIGQ") for _, b in s) <= 1
    assert any(b == "BIG" for s in seqs for _, b in s)
