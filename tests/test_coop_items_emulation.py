"""CPU tests of the item order of a heavy candidate's chunk (sage_amd/csrc/core.h: coop_items_below, coop_item_pos): where the
one-trip route of kernels.hip: score_candidates puts every (ion, fragment charge) item, one per lane.  The checks live in a
stand-alone host program, tests/hostemu/coop_items_emu.cpp (its own main; nothing of it is loaded into this process), which holds

    the positions    to the plain enumeration in (ion, charge) order — every triple of masks over 6 bits, random 64-bit triples of
                     every density, empty masks, a full M1 (N = 64, the last size the route takes) and N = 65 (the fallback);
    the item ranges  of the kind segments (kind_seg_first / kind_seg_next) to the subtract loop's kind of every ion;
    the three sums   made the route's way — a slot per item, +0.0f where an item adds nothing, every slot added four at a time — to
                     the reference's additions of the matched items alone, bit for bit, with signed zeros, denormals and values that
                     cancel among them.

This file builds the program once, runs each mode and reads its verdict."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "coop_items_emu.cpp")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coop_items") / "coop_items_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", SRC, "-o", exe])

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stdout.strip(), r.stderr.strip())
        word, cases = r.stdout.split()
        assert word == "ok"
        return int(cases)
    return run


def test_every_triple_over_six_bits(emu):
    """6-bit masks at bits 0, 29 (across the 32-bit halves) and 58 (up to bit 63)"""
    assert emu("exhaustive") == 3 * 64 ** 3


@pytest.mark.parametrize("seed", [1, 2])
def test_random_64_bit_triples(emu, seed):
    assert emu("random", seed, 100_000) == 100_000


def test_empty_full_and_fallback_sizes(emu):
    """N = 0, 64, 65, 192; bit 63 at all three charges; a charge set without the charges below it"""
    assert emu("edges") == 9


def test_segment_item_ranges(emu):
    """lm1 1 .. 70 x 1 .. 8 kinds x every chunk of the table"""
    assert emu("segments") == sum((lm1 * k + 63) // 64 for lm1 in range(1, 71) for k in range(1, 9))


def test_slot_sums_are_the_sequential_sums(emu):
    assert emu("sums", 5, 200_000) == 200_000
