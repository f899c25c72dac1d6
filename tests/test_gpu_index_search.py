"""The hand-built index cases SEARCHED on the device: tests/test_gpu_index_tables.py holds their tables to a restatement, this
module holds the kernels that READ those tables — prelim_kernel's probe and stream variants, the large-window count and replay
kernels, the precursor lookup through the peptide-mass table, the rescoring kernels' walk over the ion table — to the oracle, on
the aimed spectra of tests/index_search_worlds.py: fragment windows that end exactly on a stored m/z (which may be a cell's edge),
start inside cell 0's run of negative m/z, cover a tile without entries, lie in and beyond the table's last cell; precursor
bounds equal to a run of equal pep_mono.  tests/test_index_search_cpu.py has held the oracle to the index-free second reading on
the same worlds, so the expected values do not rest on one reading.

Every check is test_gpu_parity.check: initial_hits, every Feature field, the second step on the same handle, score_batch."""
import ctypes as C
import types

import numpy as np
import pytest

import index_search_worlds as W
import second_reading as SR
from index_reference import KIND_B, KIND_Y
from sage_amd import _lib as L
from sage_amd.api import Scorer
from test_gpu_fuzz import check_annotation, check_quick_score
from test_gpu_index_tables import GEOMETRIES, create
from test_gpu_parity import check

pytestmark = pytest.mark.gpu

INST_KINDS2, INST_BIG, INST_NONE = 2, 32, 0xFFFFFFFF
SCORER_ENV = ("SAGE_HIP_NARROW", "SAGE_HIP_WCAP")
ALL_PATHS = ("signs_by", "ties", "cell_edges_top_k256", "empty_middle")   # annotate and quick_score as well


@pytest.fixture(scope="module", params=W.NAMES)
def sw(request, gpu_required):
    return W.world(request.param)


def check_settings(w, dev, context):
    """every setting of the world on one device database; returns the first steps' timings"""
    return [check(dev, w.oracle, w.batch, p, f"{w.name}, {context}, setting {k}")[1] for k, p in enumerate(w.settings)]


def widest_window(w, params):
    """the largest `potential` (scoring.rs:351) among the world's precursor windows under `params`, from the peptide list alone"""
    ptol, widest = W.tol_tuple(params.precursor_tol), 0
    for i in range(w.batch.n):
        lo, hi = SR.bounds(ptol, W.precursor_mass(w.batch.precursor_mz[i], int(w.batch.precursor_charge[i])))
        a, b = SR.binary_search_slice(w.db.pep_mono, lo, hi)
        widest = max(widest, b - a + 1)
    return widest


@pytest.mark.parametrize("geometry", ["own", "defaults", "t6_s8"])
def test_both_index_routes(sw, geometry, monkeypatch):
    """the index built on the device from the peptide list and from host fragments; under the case's own tile geometry, the defaults
    and 64-peptide tiles with a 1/8 table — all read when the database is created"""
    env = sw.env if geometry == "own" else GEOMETRIES[geometry]
    for route, host in (("device route", sw.db), ("host route", sw.with_fragments)):
        dev = create(monkeypatch, env, host)
        check_settings(sw, dev, f"{geometry} geometry, {route}")
        dev.close()


@pytest.mark.parametrize("variant", ["stream", "probe", "tiles"])
def test_narrow_variants_and_forced_tile_kernels(sw, variant, monkeypatch):
    """SAGE_HIP_NARROW=stream walks the peptide-major list, probe reads the small tiles' succinct table; SAGE_HIP_WCAP=64 hands
    every window of more than 64 slots to the large-window count and replay kernels"""
    dev = create(monkeypatch, sw.env, sw.db)
    for var in SCORER_ENV:
        monkeypatch.delenv(var, raising=False)
    if variant != "tiles":
        # which variant ran: the stream variant walks the peptide-major list, which the index build has released and the first
        # stream batch makes again (capi_db.hip: ensure_pm_frag) — the database grows by that list; the probe variant never asks
        lib = L.load()
        before = int(lib.sage_hip_db_device_bytes(dev._h))
        monkeypatch.setenv("SAGE_HIP_NARROW", variant)
        check_settings(sw, dev, f"SAGE_HIP_NARROW={variant}")
        grown = int(lib.sage_hip_db_device_bytes(dev._h)) - before
        assert grown == (8 * (sw.ref.nf + 2) if variant == "stream" else 0), f"{sw.name}, {variant}: the database grew by {grown} bytes"
    else:
        monkeypatch.setenv("SAGE_HIP_WCAP", "64")
        timings = check_settings(sw, dev, "SAGE_HIP_WCAP=64")
        for p, t in zip(sw.settings, timings):
            if widest_window(sw, p) > 64:
                assert t["n_wide"] > 0, f"{sw.name}: windows of {widest_window(sw, p)} slots stayed in the narrow kernel"
        if sw.db.n_peptides > 64:
            assert any(widest_window(sw, p) > 64 for p in sw.settings), "the whole-database window is a large one"
    dev.close()


def test_precursor_lookup_without_the_peptide_mass_table(sw, monkeypatch):
    dev = create(monkeypatch, dict(sw.env, SAGE_HIP_NO_PEP_LUT="1"), sw.db)
    assert dev.layout()["pep_lut_bins"] == 0
    check_settings(sw, dev, "SAGE_HIP_NO_PEP_LUT=1")
    dev.close()


def test_the_rescoring_instance_the_world_is_meant_to_reach(sw, monkeypatch):
    """the instance compiled for two ion kinds for {b, y}, the general kind walks for one kind and for six, rescore_big_kernel for
    the 1 500-residue peptide of lengths_*"""
    dev = create(monkeypatch, sw.env, sw.db)
    lib, inst = L.load(), np.zeros(1, np.uint32)
    for p in sw.settings:
        scorer = Scorer(dev, p)
        scorer.score_resident(scorer.upload(sw.batch))
        L.check(lib.sage_hip_debug_rescore_instance(scorer._h, L.as_ptr(inst, C.c_uint32)))
        code = int(inst[0])
        assert code != INST_NONE, sw.name
        if sw.name.startswith("lengths"):
            assert code == INST_BIG, f"{sw.name}: instance {code:#x}"
        else:
            assert not code & INST_BIG, f"{sw.name}: instance {code:#x}"
            assert bool(code & INST_KINDS2) == (sw.kinds == [KIND_B, KIND_Y]), f"{sw.name}: kinds {sw.kinds}, instance {code:#x}"
        scorer.close()
    dev.close()


@pytest.mark.parametrize("name", ALL_PATHS)
def test_annotation_and_quick_score(name, monkeypatch, gpu_required):
    w = W.world(name)
    dev = create(monkeypatch, w.env, w.db)
    both = types.SimpleNamespace(dev=dev, orc=w.oracle)
    for k, p in enumerate(w.settings):
        ctx = f"{name}, setting {k}"
        check_annotation(both, p, w.batch, ctx)
        check_quick_score(both, p, w.batch, np.arange(0, w.batch.n, 3), ctx)
    dev.close()


def test_the_empty_database_answers_nothing(monkeypatch, gpu_required):
    """0 peptides, tables of padding only: no PSM, an empty preliminary list, nothing kept"""
    w = W.world("empty")
    dev = create(monkeypatch, w.env, w.db)
    assert dev.layout()["np"] == 0
    for p in w.settings:
        scorer = Scorer(dev, p)
        dbatch = scorer.upload(w.batch)
        packed, ln, mp, sc = scorer.initial_hits(dbatch)
        assert (mp == 0).all() and (sc == 0).all()
        for i in range(w.batch.n):  # (the reference's list of one default PreScore: potential == 1 — the oracle's, whatever it holds)
            op, omp, osc = w.oracle.initial_hits(p, w.batch, i)
            assert ln[i] == len(op) and np.array_equal(packed[i, :ln[i]], op) and (omp, osc) == (0, 0)
        gf, gc = scorer.score_resident(dbatch)
        assert (gc == 0).all()
        for low_memory in (False, True):
            keep = scorer.quick_score(dbatch, low_memory)
            assert len(keep) == 0
        scorer.close()
    dev.close()
