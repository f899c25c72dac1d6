"""The two routes of rescore_kernel: the instance compiled without chimera rounds (CHIMERA == false — what launch_rescore picks
for every search with chimera off) and the general instance (CHIMERA == true; SAGE_HIP_RESCORE_GENERAL=1, read when the scorer
is created, takes it for every search).  Same records either way, byte for byte, and the oracle's."""
import numpy as np
import pytest

from parity_utils import assert_features_equal
from sage_amd.api import DatabaseParameters, Scorer, ScorerParams, Tolerance
from sage_amd.synthetic import synthetic_fasta
from test_gpu_parity import World

pytestmark = pytest.mark.gpu

WORLDS = ("narrow", "ties", "open")
FLAGS = (None, "128", "256")  # SAGE_HIP_DEBUG_FLAGS: the dense work list, the lane-by-lane walk, the list capped at 64 items


def same_psms(fa, ca, fb, cb):
    """(features[n, report_psms], counts[n]) twice: the same records, byte for byte (slots beyond counts[i] belong to no result)"""
    if not np.array_equal(ca, cb):
        return False
    valid = np.arange(fa.shape[1])[None, :] < ca[:, None]
    return fa[valid].tobytes() == fb[valid].tobytes()


@pytest.fixture(scope="module")
def worlds(gpu_required):
    enzyme = dict(missed_cleavages=1, cleave_at="KR", restrict="P")
    # C3-like: known charges, +-10 ppm, windows of a handful of candidates
    narrow = World(synthetic_fasta(300, seed=11),
                   DatabaseParameters(bucket_size=2048, enzyme=enzyme, static_mods={"C": 57.0215}, variable_mods={"M": [15.9949]}),
                   {}, 600, seed=21)
    # tie-rich: every peptide beside its isoleucine / leucine twin (equal masses and fragments: equal hyperscores at the top)
    fasta = synthetic_fasta(60, seed=17)
    twin = fasta.replace("I", "#").replace("L", "I").replace("#", "L").replace(">sp|SYN", ">sp|TWN")
    ties = World(fasta + twin, DatabaseParameters(bucket_size=1024, enzyme=enzyme, static_mods={"C": 57.0215}), {}, 300, seed=29)
    return {
        "narrow": (narrow, narrow.batch, {}),
        "ties": (ties, ties.batch, dict(precursor_tol=Tolerance("da", -20.0, 20.0))),  # the k-select drops candidates: ties need settling
        "open": (narrow, narrow.batch.subset(np.arange(0, narrow.batch.n, 3)), dict(precursor_tol=Tolerance("da", -200.0, 200.0))),
    }


def run(world, batch, params, monkeypatch, general, flags):
    monkeypatch.delenv("SAGE_HIP_RESCORE_GENERAL", raising=False)
    monkeypatch.delenv("SAGE_HIP_DEBUG_FLAGS", raising=False)
    if general:
        monkeypatch.setenv("SAGE_HIP_RESCORE_GENERAL", "1")
    if flags:
        monkeypatch.setenv("SAGE_HIP_DEBUG_FLAGS", flags)
    scorer = Scorer(world.dev, params)  # (both variables are read here, once)
    monkeypatch.delenv("SAGE_HIP_RESCORE_GENERAL", raising=False)
    monkeypatch.delenv("SAGE_HIP_DEBUG_FLAGS", raising=False)
    gf, gc = scorer.score_resident(scorer.upload(batch))
    return gf.copy(), gc.copy(), scorer.last_timing()


@pytest.mark.parametrize("report_psms", [1, 5])
@pytest.mark.parametrize("name", WORLDS)
def test_non_chimera_search_on_both_instances(worlds, monkeypatch, name, report_psms):
    world, batch, kw = worlds[name]
    params = ScorerParams(report_psms=report_psms, **kw)
    of, oc, _, _ = world.orc.score(params, batch)
    for flags in FLAGS:
        ctx = f"{name}, report_psms={report_psms}, flags={flags}"
        df, dc, dt = run(world, batch, params, monkeypatch, False, flags)
        gf, gc, gt = run(world, batch, params, monkeypatch, True, flags)
        assert same_psms(df, dc, gf, gc), f"{ctx}: the default and the general instance differ"
        n = assert_features_equal(df, dc, of, oc, ctx + " (default instance)")
        assert assert_features_equal(gf, gc, of, oc, ctx + " (general instance)") == n
        assert n > 0, ctx
        for key in ("n_retry", "n_tied", "n_wide"):  # (the same spectra take the same routes)
            assert dt[key] == gt[key], (ctx, key)
        if name == "ties":
            assert (dt["n_tied"] if report_psms == 1 else dt["n_retry"]) > 50, ctx
        if name == "open":
            assert dt["n_wide"] > 0, ctx


@pytest.mark.parametrize("name", WORLDS)
def test_chimera_search_takes_the_general_instance_either_way(worlds, monkeypatch, name):
    world, batch, kw = worlds[name]
    params = ScorerParams(chimera=True, report_psms=3, **kw)
    of, oc, _, _ = world.orc.score(params, batch)
    df, dc, _ = run(world, batch, params, monkeypatch, False, None)
    gf, gc, _ = run(world, batch, params, monkeypatch, True, None)
    assert same_psms(df, dc, gf, gc), f"{name}, chimera: the knob changed the records"
    assert assert_features_equal(df, dc, of, oc, f"{name}, chimera") > 0
