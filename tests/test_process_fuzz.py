"""Randomised preprocessing parity: SpectrumProcessor::process (spectrum.rs:179-227, 279-412) on the host restatement
(host_db.cpp: process_ms2) and on the device (process.hip: process_kernel, through sage_hip_batch_process_upload) against the
oracle, bit for bit — masses, intensities, total ion current and peak counts.

The raw spectra come from tests/raw_spectra.py: peak counts on the kernel's edges (a wavefront, the bitonic sorts' power-of-two
padding, the LDS / global-workspace split at 2 048 raw peaks), isotope envelopes at charges 1-8, duplicated peaks, equal m/z with
different intensities, coarse and zero intensities; take_top_n and min_deisotope_mz at their edges.  Seeds are fixed: a failing
case is reproduced by its test id (and the case number in the message)."""
import os

import numpy as np
import pytest

import oracle_lib
import raw_spectra as G
from parity_utils import assert_features_equal
from sage_amd import _lib as L
from sage_amd.api import (DatabaseParameters, DeviceDatabase, RawBatch, RawSpectrum, Scorer, ScorerParams, SpectrumBatch,
                          SpectrumProcessor)
from sage_amd.synthetic import synthetic_fasta, synthetic_spectra

SALT = int(os.environ.get("SAGE_FUZZ_SALT", "2026"))


def _assert_same(got, want, context):
    gm, gi, gt = got
    om, oi, ot = want
    assert len(gm) == len(om), f"{context}: {len(gm)} peaks vs oracle {len(om)}"
    np.testing.assert_array_equal(gm, om, err_msg=f"{context}: masses")
    np.testing.assert_array_equal(gi, oi, err_msg=f"{context}: intensities")
    assert np.float32(gt) == np.float32(ot), f"{context}: total ion current {gt!r} vs oracle {ot!r}"


# ---- CPU leg: the host restatement (what the CLI runs when it preprocesses on the host) -------------------------------------
CPU_BLOCKS, CPU_CASES = 12, 125  # x 2 modes = 3 000 spectra


@pytest.mark.parametrize("deisotope", [True, False], ids=["deisotope", "heap"])
@pytest.mark.parametrize("block", range(CPU_BLOCKS))
def test_host_processing_matches_the_oracle(block, deisotope):
    for k in range(CPU_CASES):
        rng = np.random.default_rng([block, k, int(deisotope), SALT])
        n = G.peak_count(rng, huge=0.01)
        mz, it = G.raw_peaks(rng, n)
        z = G.precursor_charge(rng)
        top_n = G.take_top_n(rng, n)
        min_mz = G.min_deisotope_mz(rng, [mz])
        ctx = f"block {block} case {k}: n={n} z={z} take_top_n={top_n} min_deisotope_mz={min_mz!r}"
        p = SpectrumProcessor(top_n, deisotope, min_mz).process(RawSpectrum(mz, it, 500.0, z or None))
        _assert_same((p.masses, p.intensities, p.total_ion_current),
                     oracle_lib.process_ms2(top_n, deisotope, min_mz, mz, it, z), ctx)


# ---- GPU leg: process_kernel<false> (LDS) and process_kernel<true> (global workspace) in one batch -------------------------
GPU_CASES = 16


@pytest.fixture(scope="module")
def proc_world(gpu_required):
    host = DatabaseParameters(bucket_size=2048, enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                              static_mods={"C": 57.0215}).build(synthetic_fasta(150, seed=61))
    dev = DeviceDatabase(host, 0)
    return host, dev, oracle_lib.OracleDb.from_product(host)


def _fuzz_batch(host, rng, case):
    """About 30 raw spectra: synthetic ones (real fragment ladders, so that scoring finds PSMs) with stress peaks merged in,
    random ones at the edge counts, and 3-5 global-workspace spectra of different sizes in non-monotone order (the host sorts
    them by size before the launches: each output must land at its own index)."""
    base = synthetic_spectra(host, 14, seed=1000 + case)
    raws = []
    for k, r in enumerate(base):
        mz, it = G.raw_peaks(rng, G.peak_count(rng, huge=0.0) if k % 3 else 0)
        # (the fragment ladder above the stress peaks: a scored case still finds its PSMs after the top-N cut)
        mz, it = np.concatenate([r.mz, mz]), np.concatenate([r.intensity * np.float32(50.0), it])
        o = np.argsort(mz, kind="stable")
        z = r.precursor_charge if rng.random() < 0.7 else G.precursor_charge(rng) or None
        raws.append(RawSpectrum(mz[o], it[o], r.precursor_mz, z, r.isolation_window, r.scan_start_time, None, 0, f"syn{k}"))
    counts = [int(c) for c in rng.choice(G.EDGE_COUNTS, 10)]
    big = list(rng.choice([2049, 2100, 3001, 4096, 4097, 6000] + ([10000, 16385] if case % 4 == 1 else []), int(rng.integers(3, 6)),
                          replace=False))
    if sorted(big) == big:
        big = big[::-1]  # (never in ascending order)
    counts += [int(c) for c in big]
    for k, n in enumerate(counts):
        mz, it = G.raw_peaks(rng, n)
        raws.append(RawSpectrum(mz, it, float(np.float32(rng.uniform(350.0, 1500.0))), G.precursor_charge(rng) or None, None,
                                float(k), None, 0, f"raw{k}:{n}"))
    order = rng.permutation(len(raws))
    return [raws[i] for i in order]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(GPU_CASES))
def test_device_processing_fuzz(proc_world, case):
    """One batch per case, every spectrum against oracle_lib.process_ms2: masses, intensities, total ion current, out_npeaks;
    spectra below min_peaks keep zero peaks in the batch.  Every fourth case also scores the device-processed batch against
    the oracle scoring the oracle-processed spectra."""
    host, dev, orc = proc_world
    rng = np.random.default_rng([case, SALT])
    deisotope = case % 2 == 0
    raws = _fuzz_batch(host, rng, case)
    score = case % 4 == 0
    pick = raws[int(rng.integers(0, len(raws)))]
    top_n = int(rng.choice([63, 64, 65, 150])) if score else G.take_top_n(rng, len(pick.mz))
    min_mz = G.min_deisotope_mz(rng, [r.mz for r in raws])
    min_peaks = int(rng.choice([0, 15] if score else [0, 1, 15, 64, 65, 150]))
    ctx = f"case {case}: deisotope={deisotope} take_top_n={top_n} min_deisotope_mz={min_mz!r} min_peaks={min_peaks}"
    params = ScorerParams()
    scorer = Scorer(dev, params)
    dbatch, npk = scorer.process_upload(RawBatch(raws), take_top_n=top_n, deisotope=deisotope, min_deisotope_mz=min_mz,
                                        min_peaks=min_peaks)
    off, m, it, tic = dbatch.download()
    want = [oracle_lib.process_ms2(top_n, deisotope, min_mz, r.mz, r.intensity, r.precursor_charge) for r in raws]
    kept = []
    for i, (r, w) in enumerate(zip(raws, want)):
        c = f"{ctx}: spectrum {i} ({r.id}, {len(r.mz)} raw peaks)"
        assert npk[i] == len(w[0]), f"{c}: out_npeaks {npk[i]} vs oracle {len(w[0])}"
        a, b = int(off[i]), int(off[i + 1])
        if len(w[0]) < min_peaks:
            assert b == a, f"{c}: {b - a} peaks in the batch below min_peaks"
            continue
        kept.append(i)
        _assert_same((m[a:b], it[a:b], tic[i]), w, c)
    assert any(len(r.mz) > G.LDS_PEAKS for r in raws) and any(len(r.mz) <= G.LDS_PEAKS for r in raws)
    if not score:
        return
    gf, gc = scorer.score_resident(dbatch)
    gf, gc = gf.copy(), gc.copy()
    hb = SpectrumBatch.from_spectra([SpectrumProcessor(top_n, deisotope, min_mz).process(raws[i]) for i in kept])
    for j, i in enumerate(kept):  # (the host restatement is the oracle's, bit for bit: the CPU leg)
        assert np.array_equal(hb.masses[int(hb.peak_off[j]):int(hb.peak_off[j + 1])], want[i][0])
    of, oc, _, _ = orc.score(params, hb)
    dropped = np.setdiff1d(np.arange(len(raws)), kept)
    assert np.all(gc[dropped] == 0), f"{ctx}: PSMs for spectra below min_peaks"
    sub_f, sub_c = gf[kept].copy(), gc[kept]
    sub_f["spec_index"] = np.where(np.arange(sub_f.shape[1])[None, :] < sub_c[:, None], np.arange(len(kept))[:, None],
                                   sub_f["spec_index"])
    assert assert_features_equal(sub_f, sub_c, of, oc, f"{ctx}: device-processed batch") > 5


@pytest.mark.gpu
def test_device_processing_refuses_take_top_n_out_of_range(proc_world):
    """take_top_n is a u16 on the device (sage_hip.h): 0 and 65 536 are refused, not processed."""
    host, dev, _ = proc_world
    raws = [RawSpectrum(*G.raw_peaks(np.random.default_rng(3), 100), 600.0, 2)]
    scorer = Scorer(dev, ScorerParams())
    for top_n in (0, 65536):
        with pytest.raises(L.SageHipError, match="take_top_n"):
            scorer.process_upload(RawBatch(raws), take_top_n=top_n, deisotope=True, min_deisotope_mz=0.0, min_peaks=0)
    dbatch, npk = scorer.process_upload(RawBatch(raws), take_top_n=65535, deisotope=False, min_deisotope_mz=0.0, min_peaks=0)
    assert int(npk[0]) == 100


@pytest.mark.gpu
def test_device_processing_over_several_workspace_launches(proc_world):
    """Global-workspace spectra whose slices exceed the 1 GiB workspace budget of one launch (process.hip: the groups of
    launch_process_big): 50 spectra of ~1 M raw peaks (~51 M in all) between ordinary ones, sizes shuffled — each output at
    its own index, bit for bit.  (The heap path: deisotoping a million peaks is a serial walk of lane 0.)"""
    host, dev, _ = proc_world
    rng = np.random.default_rng([7, SALT])
    sizes = [int(s) for s in rng.integers(1_000_000, (1 << 20) + 1, 50)]
    slice_bytes = [18 * s + 4 * (1 << 20) for s in sizes]  # process.hip: process_lds_bytes
    assert sum(sorted(slice_bytes)) > (1 << 30)  # (more than one launch, whatever the grouping)
    raws = []
    for k, n in enumerate(sizes):
        mz = np.sort(rng.uniform(100.0, 2000.0, n).astype(np.float32))
        it = rng.lognormal(8.0, 1.5, n).astype(np.float32)
        raws.append(RawSpectrum(mz, it, 700.0, 2, None, 0.0, None, 0, f"huge{k}:{n}"))
        if k % 10 == 0:
            raws.append(RawSpectrum(*G.raw_peaks(rng, int(rng.choice(G.EDGE_COUNTS))), 700.0, 2, None, 0.0, None, 0, f"small{k}"))
    top_n = 150
    scorer = Scorer(dev, ScorerParams())
    dbatch, npk = scorer.process_upload(RawBatch(raws), take_top_n=top_n, deisotope=False, min_deisotope_mz=0.0, min_peaks=0)
    off, m, it, tic = dbatch.download()
    for i, r in enumerate(raws):
        w = oracle_lib.process_ms2(top_n, False, 0.0, r.mz, r.intensity, r.precursor_charge)
        assert npk[i] == len(w[0]), f"spectrum {i} ({r.id}): out_npeaks {npk[i]} vs oracle {len(w[0])}"
        a, b = int(off[i]), int(off[i + 1])
        _assert_same((m[a:b], it[a:b], tic[i]), w, f"spectrum {i} ({r.id})")
