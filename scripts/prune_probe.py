"""What there is to prune in rescore_kernel, from the oracle alone — no GPU:

    python scripts/prune_probe.py [--config C3] [--spectra 400] [--proteins 0]  > profiles/rNN_prune_probe.txt
    python scripts/prune_probe.py --gpu ...     the device's own counters over the same spectra instead (needs a GPU)

For each of the first spectra of a bench.py configuration: the preliminary list (OracleDb.initial_hits) and, for each listed
candidate, its exact matched_b + matched_y (OracleDb.brute_force).  A candidate below min_matched_peaks fails scoring.rs:491 and
contributes nothing to any result; the device drops it behind the bitmap filter when its matches so far plus the items the bitmap
lets through stay below the bound (the exact count plus the bitmap's false positives).  The profiling instance's counters over
the same spectra (--gpu: sage_hip_debug_prune_counters) belong beside this table."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def candidate_matches(orc, params, batch, i):
    """exact matched_b + matched_y of every valid candidate of spectrum i's preliminary list"""
    packed, _, _ = orc.initial_hits(params, batch, i)
    windows, matched = {}, []
    for word in packed:
        word = int(word)
        pep, z, iso = (word >> 16) & 0xFFFFFFFF, (word >> 8) & 0xFF, (word & 0xFF) - 128
        if pep == 0xFFFFFFFF or (word >> 48) == 0:
            continue
        if (z, iso) not in windows:
            p, m, _ = orc.brute_force(params, batch, i, z, iso, cap=1 << 20)
            windows[(z, iso)] = dict(zip(p.tolist(), m.tolist()))
        matched.append(windows[(z, iso)][pep])
    return np.array(matched, dtype=np.int64)


def gpu_counters(args, host, params, batch):
    import ctypes as C

    from sage_amd import _lib as L
    from sage_amd.api import DeviceDatabase, Scorer
    os.environ["SAGE_HIP_PHASE_CLOCKS"] = "1"
    scorer = Scorer(DeviceDatabase(host, 0), params)
    del os.environ["SAGE_HIP_PHASE_CLOCKS"]
    _, counts = scorer.score_resident(scorer.upload(batch))
    out = np.zeros(4, np.uint64)
    L.check(L.load().sage_hip_debug_prune_counters(scorer._h, L.as_ptr(out, C.c_uint64)))
    t = scorer.last_timing()
    n = batch.n
    print(f"# {args.config}: first {n} spectra on the device (profiling instance), {int(counts.sum())} PSMs, n_retry {t['n_retry']}, n_tied {t['n_tied']}")
    print(f"candidates pruned                             {int(out[0])} ({out[0] / n:.1f} per spectrum)")
    print(f"(ion, charge) items pruned                    {int(out[1])} ({out[1] / n:.1f} per spectrum)")
    print(f"scoring rounds that left early                {int(out[2])} of {n}")
    print(f"rounds with a passing candidate beside pruned {int(out[3])} of {n}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--spectra", type=int, default=400)
    ap.add_argument("--proteins", type=int, default=0)
    ap.add_argument("--gpu", action="store_true", help="score the same spectra on device 0 and print the profiling instance's prune counters")
    args = ap.parse_args()
    import oracle_lib
    from sage_amd.workloads import CONFIGS, build_host_db, scorer_params, workload_batch
    cfg = CONFIGS[args.config]
    host = build_host_db(cfg, args.proteins or None)
    params = scorer_params(cfg)
    batch, _ = workload_batch(cfg, host, 0, args.spectra)
    if args.gpu:
        return gpu_counters(args, host, params, batch)
    orc = oracle_lib.OracleDb.from_product(host)
    need = params.min_matched_peaks
    n_valid = n_pass = all_m = pruned_m = top_m = 0
    none_valid = nobody = one_passer = 0
    hist = np.zeros(7, np.int64)
    for i in range(batch.n):
        m = candidate_matches(orc, params, batch, i)
        if len(m) == 0:
            none_valid += 1
            continue
        n_valid += len(m)
        n_pass += int((m >= need).sum())
        all_m += int(m.sum())
        pruned_m += int(m[m < need].sum())
        top_m += int(m.max()) if m.max() >= need else 0
        nobody += int(m.max() < need)
        one_passer += int((m >= need).sum() == 1)
        hist += np.bincount(np.minimum(m, 6), minlength=7)
    n = batch.n
    print(f"# {args.config}: first {n} spectra against {host.n_peptides} peptides, min_matched_peaks {need}, report_psms {params.report_psms}")
    print(f"valid candidates per spectrum                 {n_valid / n:.1f}")
    print(f"candidates per spectrum with matched >= {need}      {n_pass / n:.1f}")
    print(f"candidates per spectrum that cannot pass      {(n_valid - n_pass) / n:.1f} ({100.0 * (n_valid - n_pass) / max(n_valid, 1):.0f} %)")
    print(f"histogram of matched = 0 / 1 / 2 / 3 / 4 / 5 / >= 6   {' / '.join(str(int(v)) for v in hist)}")
    print(f"all matches                                   {all_m}")
    print(f"matches in candidates that cannot pass        {pruned_m} ({100.0 * pruned_m / max(all_m, 1):.0f} %)")
    print(f"matches in each spectrum's top candidate      {top_m} ({100.0 * top_m / max(all_m, 1):.0f} %)")
    print(f"matches in the other passing candidates       {all_m - pruned_m - top_m}")
    print(f"spectra with no valid candidate               {none_valid} of {n}")
    print(f"spectra with valid candidates, none can pass  {nobody} of {n} ({100.0 * nobody / n:.0f} %)")
    print(f"spectra in which exactly one candidate passes {one_passer} of {n} ({100.0 * one_passer / n:.0f} %)")


if __name__ == "__main__":
    main()
