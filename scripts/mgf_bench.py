#!/usr/bin/env python3
"""MGF input at a user's size, beside the mzML reader, and the wide-window step with ppm isolation windows beside the same
step with Da windows.  Prints one JSON line:
  * read: the same S synthetic spectra of P peaks written once as MGF (text peaks) and once as mzML (32-bit zlib arrays), each
    read by its C++ reader (sage_hip_mgf_read / sage_hip_mzml_read) on SAGE_HIP_THREADS host threads (default 16): median
    seconds, spectra/s and MB/s of the file as stored;
  * wide_window: one resident batch of W synthetic spectra, scored with wide_window on (sage_hip_score_resident), its isolation
    windows once as Da(-w, w) and once as Ppm(-w', w') with w' = w * 1e6 / precursor m/z (the same width at the precursor):
    median milliseconds per step and PSMs.

    python scripts/mgf_bench.py [--spectra 100000 --peaks 150 --wide 20000 --steps 5]
"""
import argparse
import json
import os
import sys
import tempfile
import time

os.environ.setdefault("SAGE_HIP_THREADS", "16")
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sage_amd.api import RawSpectrum  # noqa: E402
from sage_amd.mgf import read_mgf_native, write_mgf  # noqa: E402
from sage_amd.mzml import read_mzml_native, write_mzml  # noqa: E402

F32 = np.float32


def spectra(n, peaks, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        mz = np.sort(rng.uniform(100.0, 2000.0, peaks)).astype(F32)
        it = rng.lognormal(8.0, 1.5, peaks).astype(F32)
        secs = F32(rng.uniform(0.0, 7200.0))
        out.append(RawSpectrum(mz, it, float(F32(rng.uniform(350.0, 1500.0))), int(rng.integers(2, 5)), (-1.0, 1.0),
                               float(secs / F32(60.0)), id=f"controllerType=0 controllerNumber=1 scan={i + 1}"))
    return out


def timed(fn, steps):
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def read_leg(args, tmp):
    sp = spectra(args.spectra, args.peaks)
    mgf, mzml = os.path.join(tmp, "bench.mgf"), os.path.join(tmp, "bench.mzML")
    write_mgf(mgf, sp)
    write_mzml(mzml, sp)
    assert read_mgf_native(mgf)[0].n == read_mzml_native(mzml).n == args.spectra
    out = {}
    for name, path, fn in (("mgf", mgf, lambda: read_mgf_native(mgf)), ("mzml", mzml, lambda: read_mzml_native(mzml))):
        fn()  # (page cache)
        s = timed(fn, args.steps)
        mb = os.path.getsize(path) / 1e6
        out[name] = {"seconds": s, "spectra_per_s": args.spectra / s, "file_mb": mb, "mb_per_s": mb / s}
    return out


def wide_leg(args):
    from sage_amd.api import DatabaseParameters, DeviceDatabase, Scorer, ScorerParams, SpectrumBatch, SpectrumProcessor
    from sage_amd.synthetic import synthetic_fasta, synthetic_spectra
    host = DatabaseParameters(enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                              static_mods={"C": 57.0215}).build(synthetic_fasta(2000, seed=5))
    rng = np.random.default_rng(6)
    proc = SpectrumProcessor(150, True, 0.0)
    sp = []
    for r in synthetic_spectra(host, args.wide, seed=7):
        w = float(F32(rng.uniform(0.5, 2.0)))
        sp.append(proc.process(RawSpectrum(r.mz, r.intensity, r.precursor_mz, r.precursor_charge, (-w, w), r.scan_start_time)))
    da = SpectrumBatch.from_spectra(sp)
    ppm = SpectrumBatch.from_spectra(sp)
    ppm.isolation_lo = np.ascontiguousarray(da.isolation_lo * F32(1e6) / da.precursor_mz, dtype=F32)
    ppm.isolation_hi = np.ascontiguousarray(da.isolation_hi * F32(1e6) / da.precursor_mz, dtype=F32)
    scorer = Scorer(DeviceDatabase(host, 0), ScorerParams(wide_window=True, report_psms=1))
    out = {}
    for name, batch, kinds in (("da", da, None), ("ppm", ppm, np.zeros(da.n, np.uint8))):
        dbatch = scorer.upload(batch, iso_kind=kinds)
        scorer.score_resident(dbatch)  # (warm-up)
        s = timed(lambda: scorer.score_resident(dbatch), args.steps)
        _, counts = scorer.score_resident(dbatch)
        out[name] = {"ms_per_step": s * 1e3, "spectra": int(da.n), "psms": int(counts.sum())}
        dbatch.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=100000)
    ap.add_argument("--peaks", type=int, default=150)
    ap.add_argument("--wide", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-gpu", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        res = {"threads": int(os.environ["SAGE_HIP_THREADS"]), "spectra": args.spectra, "peaks": args.peaks, "read": read_leg(args, tmp)}
    if not args.no_gpu:
        res["wide_window"] = wide_leg(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
