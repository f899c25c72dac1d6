"""One scorer handle held to the oracle across sequences of DIFFERENT steps, as the command line drives it (cli.search_file: one
handle per device for the whole run, file after file) — the state a handle carries from step to step in csrc/capi.hip:
retry_likely and the deferred retry pass with its late launch (resident_attempt / launch_deferred_retries / enqueue_late_retry / collect_retry),
per part of a step in parts; counters_clean; the timing interval (steps without events); page-locked and pageable result arrays;
working sets that grow and shrink; outs[] shared by the parts of a resident step and the lanes of the streaming entry; large-window
batches behind narrow ones; a wrongly guessed step in parts repeated as one; the entry points that put `timed` back.

ONE invariant: a step's results do not depend on what the handle did before.  tests/handle_sequences.py holds every scoring step to
the oracle (initial_hits, quick_score and annotate to theirs; score_candidates and localise byte for byte to the same calls on a fresh
handle), every resident step's n_retry / n_wide / n_ways to a fresh handle's first step on the same batch, and its total_ms to the
timing interval.  n_launches is compared with a fresh handle's first step (which always launches its retry pass), less one per
part that left the pass out — never with a literal.  tests/test_handle_sequences_cpu.py holds the world to what is assumed here.

Wall time per test on the MI355X, 5.0 s for the 25 tests: the module fixture (world, device database) 0.90 s; the fresh handles of
the reach test 0.64 s (it measures most batches first); drawn sequences 0.09 to 0.28 s each; the sequences in parts 0.17 to
0.20 s; the command line's loop 0.13 s; every other test 0.04 to 0.10 s.  A second run, on a machine busy with other work, took
33 s, every test about seven times as long: the slowest were drawn sequence 0 with 5.5 s (it is the first to ask the oracle for
the annotations of Q and R) and the reach test with 4.3 s; no other test was above 2.8 s.  The repeated step's sequence, added
since: 0.28 s asked for two parts, 0.42 to 0.51 s for three; the module's 27 tests 8.7 s."""
import numpy as np
import pytest

import handle_sequences as H
from parity_utils import assert_features_equal
from sage_amd.api import DeviceDatabase

pytestmark = pytest.mark.gpu

FIRST = ["Q", "Q2", "R", "R", "Q", "R", "E", "R", "S1", "Q", "S65"]


@pytest.fixture(scope="module")
def env(gpu_required):
    w = H.world()
    dev = DeviceDatabase(w.host, 0)
    return w, dev, H.Fresh(w, dev)


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in ("SAGE_HIP_WAYS", "SAGE_HIP_CHUNK", "SAGE_HIP_EXACT", "SAGE_HIP_NO_ZEROCOPY"):
        monkeypatch.delenv(k, raising=False)


def handle(env, cfg="main", label=""):
    w, dev, fresh = env
    h = H.Handle(w, cfg, dev, fresh)
    h.label = label
    return h


def test_fresh_handles_reach_what_the_sequences_need(env, monkeypatch):
    """The reach conditions, on fresh handles: the quiet batches retry nothing, R at least 50 spectra, the mixed ones some; BIG goes
    in two parts by default and in three when asked; W takes the large-window kernels and N does not."""
    _, _, fresh = env
    for name in ("Q", "Q2", "BIGQ"):
        assert fresh("main", name)["n_retry"] == 0 and fresh("main", name)["n_wide"] == 0, name
    assert fresh("main", "R")["n_retry"] >= 50 and fresh("main", "R")["n_wide"] == 0
    assert fresh("main", "S65")["n_retry"] > 0 and fresh("main", "S1")["n_retry"] > 0 and fresh("main", "BIG")["n_retry"] > 0
    assert fresh("main", "BIG")["n_ways"] == 2 == fresh("main", "BIGQ")["n_ways"] and fresh("main", "R")["n_ways"] == 1
    assert fresh("main", "R")["candidates"][0] >= 20  # (candidate lists that are not empty)
    assert fresh("second", "N")["n_retry"] == 0 and fresh("second", "N")["n_wide"] == 0
    assert fresh("second", "W")["n_retry"] > 10 and fresh("second", "W")["n_wide"] > 0
    monkeypatch.setenv("SAGE_HIP_WAYS", "3")
    assert fresh("main", "BIG")["n_ways"] == 3 == fresh("main", "BIGQ")["n_ways"]
    assert fresh("main", "BIG")["n_retry"] > 0 and fresh("main", "BIGQ")["n_retry"] == 0


def check_first_sequence(fresh, ts):
    """n_launches along FIRST: which steps left their retry pass out, against a fresh handle's first step on the same batch"""
    first = lambda name: fresh("main", name)["n_launches"]
    assert ts[0]["n_launches"] == first("Q"), "the first step of a handle launches its retry pass"
    assert ts[1]["n_launches"] == first("Q2") - 1, "a quiet step behind a quiet step launches no retry pass: the next one starts deferred"
    assert ts[2]["n_launches"] == first("R"), "deferred, retries found: the pass launched late, and collect_retry counted it"
    for k in (2, 5, 7, 10):  # the late launches: the pass's own time is in the step's figures when the step has events
        assert not ts[k]["timed"] or ts[k]["retry_ms"] > 0.0, (k, ts[k])
    assert ts[3]["n_launches"] == first("R"), "not deferred"
    assert ts[4]["n_launches"] == first("Q"), "not deferred behind a step with retries"
    assert ts[5]["n_launches"] == first("R") and ts[7]["n_launches"] == first("R")
    assert ts[9]["n_launches"] == first("Q"), "not deferred behind S1's retry"
    assert ts[10]["n_launches"] == first("S65")
    assert ts[2]["records"] == ts[3]["records"] == ts[5]["records"] == ts[7]["records"]
    assert ts[0]["records"] == ts[4]["records"] == ts[9]["records"]


def test_late_launch_in_one_part(env):
    """Q Q2 R R Q R E R S1 Q S65: the R behind Q2 takes the late route (Q2 launched no retry pass, so R starts deferred and finds
    retries), the second R goes undeferred, E is an empty step behind a step with retries and ahead of a deferred one."""
    h = handle(env)
    check_first_sequence(env[2], h.run([("pinned", b) for b in FIRST]))


def parts_sequence(env, steps, n_ways):
    _, _, fresh = env
    h = handle(env)
    ts = h.run(steps)
    big = [(k, t) for k, ((_, b), t) in enumerate(zip(steps, ts)) if b in ("BIG", "BIGQ")]
    assert all(t["n_ways"] == n_ways for _, t in big)
    return ts, lambda name: fresh("main", name)["n_launches"]


def test_late_launch_in_three_parts(env, monkeypatch):
    """BIGQ BIGQ BIG BIG BIGQ BIG in three parts: the first BIG starts deferred in every part and only the parts that hold R spectra
    launch their retry pass late; the second BIG launches it in every part."""
    monkeypatch.setenv("SAGE_HIP_WAYS", "3")
    ts, first = parts_sequence(env, [("pinned", b) for b in ("BIGQ", "BIGQ", "BIG", "BIG", "BIGQ", "BIG")], 3)
    assert ts[0]["n_launches"] == first("BIGQ")
    assert ts[1]["n_launches"] == first("BIGQ") - 3, "no part launched a retry pass"
    assert first("BIG") - 3 < ts[2]["n_launches"] < first("BIG"), "the late launch in some parts and not in others"
    assert ts[3]["n_launches"] == first("BIG") and ts[4]["n_launches"] == first("BIGQ")
    assert first("BIG") - 3 < ts[5]["n_launches"] < first("BIG")
    assert ts[2]["records"] == ts[3]["records"] == ts[5]["records"]


def test_late_launch_in_two_parts_and_back_to_one(env):
    """The same with the default two parts at this size, Q and R in between: the step falls back to one part, the working set is
    used at 300 spectra and at 24 576 again."""
    ts, first = parts_sequence(env, [("pinned", b) for b in ("BIGQ", "BIGQ", "BIG", "Q", "R", "BIG", "BIGQ", "Q", "BIG")], 2)
    assert ts[1]["n_launches"] == first("BIGQ") - 2
    assert ts[2]["n_launches"] == first("BIG") - 1, "one of two parts launched late"
    assert ts[3]["n_launches"] == first("Q") and ts[4]["n_launches"] == first("R")  # (Q behind BIG: not deferred; R behind Q: late)
    assert ts[5]["n_launches"] == first("BIG") and ts[7]["n_launches"] == first("Q") - 1
    assert ts[8]["n_launches"] == first("BIG") - 1
    assert ts[2]["records"] == ts[5]["records"] == ts[8]["records"]


@pytest.mark.parametrize("every", [0, 3])
def test_steps_without_events(env, every):
    """FIRST under set_timing_interval(0) and (3): records, n_retry and the launches as with events; total_ms 0 on the steps without
    events and above 0 on the others (H.Handle.step); a quick_score and an initial_hits step between two steps without events —
    they record their own events and put `timed` back."""
    h = handle(env)
    steps = [("timing", every)] + [("pinned", b) for b in FIRST]
    steps.insert(3, ("quick0", "S65"))  # between Q2 and R (resident steps 1 and 2)
    steps.insert(7, ("hits", "S1"))     # between Q and R (resident steps 4 and 5)
    ts = [t for t in h.run(steps) if t is not None]
    check_first_sequence(env[2], ts)
    timed = [t["timed"] for t in ts]
    assert timed == [every != 0 and k % every == 0 for k in range(len(FIRST))]
    assert not (timed[1] or timed[2] or timed[4] or timed[5])


def test_page_locked_and_pageable_results_alternate(env):
    """Q(pinned) R(pageable) Q(pinned) Q2(pinned) R(pinned) R(pageable) Q(pageable) R(pinned): a pageable step has no epilogue (its
    counters stay dirty, it cannot defer), a page-locked one behind it must zero them itself."""
    h = handle(env)
    ts = h.run([("pinned", "Q"), ("pageable", "R"), ("pinned", "Q"), ("pinned", "Q2"), ("pinned", "R"), ("pageable", "R"),
                ("pageable", "Q"), ("pinned", "R")])
    assert ts[1]["records"] == ts[4]["records"] == ts[5]["records"] == ts[7]["records"]
    assert ts[0]["records"] == ts[2]["records"] == ts[6]["records"]


def test_page_locked_and_pageable_results_alternate_in_three_parts(env, monkeypatch):
    monkeypatch.setenv("SAGE_HIP_WAYS", "3")
    ts, _ = parts_sequence(env, [("pinned", "BIGQ"), ("pageable", "BIG"), ("pinned", "BIGQ"), ("pinned", "BIGQ"), ("pinned", "BIG"),
                                 ("pageable", "BIG"), ("pageable", "BIGQ"), ("pinned", "BIG")], 3)
    assert ts[1]["records"] == ts[4]["records"] == ts[5]["records"] == ts[7]["records"]


def test_the_command_lines_loop_twice_over_three_files(env):
    """process_upload -> score_resident -> annotate -> score_candidates -> localise -> close per file (Q, R, S65 as raw spectra),
    two passes on one handle: every output held as everywhere, the second pass's byte-equal to the first's."""
    h = handle(env)
    files = [("process", "Q"), ("process", "R"), ("process", "S65")]
    one, two = h.run(files), h.run(files)
    for a, b, (_, name) in zip(one, two, files):
        for k in ("records", "annotation", "candidates"):
            assert a[k] == b[k], f"{k} of {name} differ between the passes"
    assert one[1]["candidates"][0] >= 20


@pytest.mark.parametrize("chunk", [None, "128"])
def test_streaming_between_resident_steps(env, monkeypatch, chunk):
    """Q(resident) R(score) Q2(resident) R(resident): the streaming entry uses the same outs[] and working sets, in one chunk and
    in three."""
    if chunk:
        monkeypatch.setenv("SAGE_HIP_CHUNK", chunk)
    h = handle(env)
    ts = h.run([("pinned", "Q"), ("stream", "R"), ("pinned", "Q2"), ("pinned", "R"), ("stream", "S65"), ("stream", "E"), ("pinned", "R")])
    assert ts[3]["records"] == ts[6]["records"]


def test_a_clone_keeps_its_own_state(env):
    """Steps alternate between a handle and its clone: a quiet on the handle, R on the clone.  The handle's second Q leaves its
    retry pass out although the clone has just retried; the clone's Q2 launches it although the handle's Q found nothing."""
    _, _, fresh = env
    first = lambda name: fresh("main", name)["n_launches"]
    a = handle(env, label="handle")
    b = a.fork("clone")
    a0, b0, a1, b1 = a.step("pinned", "Q"), b.step("pinned", "R"), a.step("pinned", "Q"), b.step("pinned", "R")
    assert a0["n_launches"] == first("Q") and a1["n_launches"] == first("Q") - 1
    assert b0["n_launches"] == first("R") == b1["n_launches"] and b0["records"] == b1["records"]
    a2, b2, b3 = a.step("pinned", "R"), b.step("pinned", "Q2"), b.step("pinned", "Q")
    assert a2["records"] == b0["records"] and a2["n_launches"] == first("R")
    assert b2["n_launches"] == first("Q2") and b3["n_launches"] == first("Q") - 1


def test_large_windows_behind_narrow_steps_and_back(env):
    """N W N N W W N under the second configuration: n_wide above 0 exactly on the W steps."""
    h = handle(env, "second")
    names = ["N", "W", "N", "N", "W", "W", "N"]
    ts = h.run([("pinned", b) for b in names])
    for name, t in zip(names, ts):
        assert (t["n_wide"] > 0) == (name == "W"), (name, t["n_wide"])
        assert t["n_retry"] > 10 if name == "W" else t["n_retry"] == 0
    assert ts[1]["records"] == ts[4]["records"] == ts[5]["records"] and ts[0]["records"] == ts[2]["records"] == ts[6]["records"]


@pytest.mark.parametrize("ways", [None, "3"])
def test_a_wrong_guess_in_parts_is_repeated_as_one(env, monkeypatch, ways):
    """BIG under the second configuration, uploaded with SAGE_HIP_ASSUME_NARROW=1 (the upload then says "no large windows" and
    skips the exact check): the step starts without the large-window kernels, its twin spectra queue for them, and the step is
    repeated as ONE part with them (score_resident_locked).  Then N, the SAME device batch again — it now remembers maybe_wide —
    and W.  Every step matches the oracle; the repeated step reports what a fresh handle reports for a batch known to be wide
    (n_wide > 0, one part, both passes' launches: the first attempt leaves nothing in the figures); the second BIG step matches
    the first byte for byte; N behind it is a fresh handle's N, launches included.
    ASSUMED, not observed: that the first attempt went in two parts (three with SAGE_HIP_WAYS=3).  It follows from
    resident_attempt — 24 576 >= 8192 x parts and maybe_wide == false — but n_ways is the repeated attempt's and the
    SAGE_HIP_STEP_TRACE line does not name the parts.  tests/test_handle_sequences_cpu.py holds the windows to what is needed."""
    w, _, fresh = env
    if ways:
        monkeypatch.setenv("SAGE_HIP_WAYS", ways)
    want, want_n = fresh("second", "BIG"), fresh("second", "N")  # (measured without the switch: the upload's exact check says "wide")
    assert want["n_wide"] > 0 and want["n_ways"] == 1 and want["n_retry"] > 0
    h = handle(env, "second")
    batch, oracle = w.batch("BIG"), w.oracle("second", "BIG")
    monkeypatch.setenv("SAGE_HIP_ASSUME_NARROW", "1")
    dbatch = h.scorer.upload(batch)
    try:
        gf, gc, t1 = h._resident(dbatch, batch.n)
        monkeypatch.delenv("SAGE_HIP_ASSUME_NARROW")
        assert_features_equal(gf, gc, *oracle, "BIG, the repeated step")
        assert t1["n_wide"] > 0 and t1["n_ways"] == 1, t1
        assert {k: t1[k] for k in ("n_retry", "n_launches", "n_wide", "n_ways")} == {k: want[k] for k in ("n_retry", "n_launches", "n_wide", "n_ways")}
        first = H.valid_bytes(gf, gc)
        tn = h.step("pinned", "N")  # (held to the oracle and to a fresh handle's n_retry / n_wide / n_ways in Handle.step)
        assert tn["n_launches"] == want_n["n_launches"], "N behind a step with retries launches its retry pass, like a fresh handle"
        monkeypatch.setenv("SAGE_HIP_ASSUME_NARROW", "1")
        gf, gc, t3 = h._resident(dbatch, batch.n)
        monkeypatch.delenv("SAGE_HIP_ASSUME_NARROW")
        assert_features_equal(gf, gc, *oracle, "BIG again")
        assert H.valid_bytes(gf, gc) == first
        assert {k: t3[k] for k in ("n_retry", "n_launches", "n_wide", "n_ways")} == {k: want[k] for k in ("n_retry", "n_launches", "n_wide", "n_ways")}
    finally:
        dbatch.close()
    tw = h.step("pinned", "W")
    assert tw["n_wide"] > 0 and tw["n_retry"] > 10


@pytest.mark.parametrize("seed", range(12))
def test_drawn_sequences(env, monkeypatch, seed):
    """Fourteen steps drawn from the alphabet (H.draw_sequence(seed)); every third seed in three parts, every second with the
    streaming entry in chunks of 128.  A failure names the seed and the steps up to the failing one."""
    if seed % 3 == 0:
        monkeypatch.setenv("SAGE_HIP_WAYS", "3")
    if seed % 2 == 1:
        monkeypatch.setenv("SAGE_HIP_CHUNK", "128")
    handle(env, label=f"seed {seed}:").run(H.draw_sequence(seed))
