"""What the cooperative ("heavy candidates") path of rescore_kernel's score_candidates walks per spectrum, from the
oracle's lists — no GPU:

    python scripts/heavy_probe.py [--config C3] [--spectra 600] [--proteins 0]  > profiles/rNN_heavy_probe.txt
    python scripts/heavy_probe.py --gpu ...     the device's own counters over the same spectra instead (needs a GPU)

For each of the first spectra of a bench.py configuration: the preliminary list (OracleDb.initial_hits) and, for every valid
candidate, its b / y ion table restated here (residue masses and modifications of the host database), the peak-presence bitmap's
hits per 64-ion chunk and fragment charge (core.h: pbm_index / pbm_peak_span, restated) and the exact matches (|peak - m/z| within
the fragment tolerance; checked against OracleDb.brute_force's matched counts below).  The kernel's rules: a candidate on its last
chunk whose matches so far plus its hits stay below min_matched_peaks is pruned; a candidate with more than COOP_MIN_HITS hits in a
chunk is taken by the whole wavefront when at most COOP_MAX_LANES candidates of the spectrum's chunk are that heavy.  For the
chunks taken that way: the bits of K1 | K2 | K3 the add loop walks, its (ion, charge) items, the kind segments that hold a bit and
the runs of consecutive matched ions within them — what run_matched_mask (core.h) updates a run state once for.
The profiling instance's counters over the same spectra (--gpu: sage_hip_debug_heavy_counters) belong beside this table."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COOP_MIN_HITS, COOP_MAX_LANES = 12, 2  # kernels.hip: SAGE_COOP_MIN_HITS, SAGE_COOP_MAX_LANES
PBM_BITS, PBM_INV_W = 1 << 15, 16.0    # core.h


def gpu_counters(args, host, params, batch):
    import ctypes as C

    from sage_amd import _lib as L
    from sage_amd.api import DeviceDatabase, Scorer
    os.environ["SAGE_HIP_PHASE_CLOCKS"] = "1"
    scorer = Scorer(DeviceDatabase(host, 0), params)
    del os.environ["SAGE_HIP_PHASE_CLOCKS"]
    _, counts = scorer.score_resident(scorer.upload(batch))
    out = np.zeros(2, np.uint64)
    L.check(L.load().sage_hip_debug_heavy_counters(scorer._h, L.as_ptr(out, C.c_uint64)))
    t = scorer.last_timing()
    n = batch.n
    print(f"# {args.config}: first {n} spectra on the device (profiling instance), {int(counts.sum())} PSMs, n_retry {t['n_retry']}, n_tied {t['n_tied']}"
          f" (a spectrum of the retry pass is scored twice)")
    print(f"chunks of heavy candidates taken together     {int(out[0])} ({out[0] / n:.2f} per spectrum)")
    print(f"(ion, charge) matches added up for them       {int(out[1])} ({out[1] / n:.2f} per spectrum)")
    routes = np.zeros(2, np.uint64)
    L.check(L.load().sage_hip_debug_heavy_routes(scorer._h, L.as_ptr(routes, C.c_uint64)))
    print(f"... in one lookup trip, sums from LDS         {int(routes[0])} ({100.0 * routes[0] / max(int(out[0]), 1):.2f} %)")
    print(f"... a trip per fragment charge (fallback)     {int(routes[1])} ({100.0 * routes[1] / max(int(out[0]), 1):.2f} %: more than 64 items, or not the last chunk)")


def bitmap_of(peaks, tol):
    """core.h: pbm_reach_of / pbm_peak_span, in double (a probe: a bin's edge may fall either way)"""
    tmax = max(abs(tol.lo), abs(tol.hi))
    rel = tmax * 1e-6 if tol.kind == "ppm" else tmax * 1e-2 if tol.kind == "pct" else 0.0
    a = rel / (1.0 - rel) * 1.0002 + 2.0 ** -20
    b = (tmax * 1.0002 if tol.kind == "da" else 0.0) + 2.0 ** -20
    bm = np.zeros(PBM_BITS, bool)
    d = peaks * a + b
    for b0, b1 in zip(np.floor((peaks - d) * PBM_INV_W).astype(np.int64), np.floor((peaks + d) * PBM_INV_W).astype(np.int64)):
        bm[np.arange(max(b0, 0), b1 + 1) % PBM_BITS] = True
    return bm


def runs_of(bits):
    """maximal runs of consecutive True in a boolean vector"""
    return int(np.count_nonzero(bits & ~np.concatenate(([False], bits[:-1]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--spectra", type=int, default=600)
    ap.add_argument("--proteins", type=int, default=0)
    ap.add_argument("--gpu", action="store_true", help="score the same spectra on device 0 and print the profiling instance's counters of the path")
    args = ap.parse_args()
    import oracle_lib
    from sage_amd import _lib as L
    from sage_amd.synthetic import _MASS_LUT
    from sage_amd.workloads import CONFIGS, build_host_db, scorer_params, workload_batch
    cfg = CONFIGS[args.config]
    host = build_host_db(cfg, args.proteins or None)
    params = scorer_params(cfg)
    batch, _ = workload_batch(cfg, host, 0, args.spectra)
    if args.gpu:
        return gpu_counters(args, host, params, batch)
    kinds = [k for k, v in L.ION_KINDS.items() for c in host.ion_kinds.tolist() if v == c]
    assert kinds == ["b", "y"], f"the probe restates the b and y series only, not {kinds}"
    tol = params.fragment_tol
    assert tol.kind == "ppm"
    orc = oracle_lib.OracleDb.from_product(host)
    seq_off = host.seq_off.astype(np.int64)
    peak_off = batch.peak_off.astype(np.int64)
    need = params.min_matched_peaks
    n = batch.n
    taken = bits = items = segs = runs = pruned = crowded = with_path = single_charge_segs = 0
    top_items = []
    checked = agree = 0
    for i in range(n):
        packed, _, _ = orc.initial_hits(params, batch, i)
        peaks = batch.masses[peak_off[i]:peak_off[i + 1]].astype(np.float64)
        bm = bitmap_of(peaks, tol)
        cands, windows = [], {}
        for word in packed:
            word = int(word)
            pep, z, iso = (word >> 16) & 0xFFFFFFFF, (word >> 8) & 0xFF, (word & 0xFF) - 128
            if pep == 0xFFFFFFFF or (word >> 48) == 0:
                continue
            a, b = seq_off[pep], seq_off[pep + 1]
            res = _MASS_LUT[host.seq[a:b]] + host.mods[a:b].astype(np.float64)
            nterm = float(host.nterm[pep]) if not np.isnan(host.nterm[pep]) else 0.0
            bs = nterm + np.cumsum(res)[:-1]
            ions = np.concatenate([bs, float(host.pep_mono[pep]) - bs])
            nfz = z - 1 if params.max_fragment_charge is None else min(z - 1, params.max_fragment_charge)
            if nfz < 1 or nfz > 3 or len(bs) == 0:
                continue  # (charges above 3 are not filtered and never take the path)
            x = np.floor(ions * PBM_INV_W).astype(np.int64)
            hit = np.stack([bm[(x // c) % PBM_BITS] for c in range(1, nfz + 1)])
            mz = ions[None, :] / np.arange(1, nfz + 1)[:, None]
            lo, hi = mz * (1.0 + tol.lo * 1e-6), mz * (1.0 + tol.hi * 1e-6)
            ok = ((peaks[None, None, :] >= lo[:, :, None]) & (peaks[None, None, :] <= hi[:, :, None])).any(axis=2)
            ok &= hit  # (the bitmap never drops a match; in double a bin's edge may, once in a long while)
            if (z, iso) not in windows:
                p, m, _ = orc.brute_force(params, batch, i, z, iso, cap=1 << 20)
                windows[(z, iso)] = dict(zip(p.tolist(), m.tolist()))
            checked += 1
            agree += int(windows[(z, iso)][pep] == int(ok.sum()))
            cands.append((len(bs), hit, ok))
        any_taken = False
        top = 0
        longest = max((2 * lm1 for lm1, _, _ in cands), default=0)
        so_far = [0] * len(cands)
        for j0 in range(0, longest, 64):
            hc = []
            for c, (lm1, hit, ok) in enumerate(cands):
                h = int(hit[:, j0:j0 + 64].sum())
                if h and j0 + 64 >= 2 * lm1 and so_far[c] + h < need:
                    pruned += 1
                    h = 0
                hc.append(h)
            heavy = [c for c, h in enumerate(hc) if h > COOP_MIN_HITS]
            if len(heavy) > COOP_MAX_LANES:
                crowded += 1
                heavy = []
            for c in heavy:
                lm1, hit, ok = cands[c]
                k = ok[:, j0:j0 + 64]
                anyk = k.any(axis=0)
                taken += 1
                any_taken = True
                bits += int(anyk.sum())
                items += int(k.sum())
                top += int(k.sum())
                for kind in range(2):  # the chunk's kind segments
                    lo_bit, hi_bit = max(kind * lm1 - j0, 0), min((kind + 1) * lm1 - j0, 64)
                    if hi_bit > lo_bit and anyk[lo_bit:hi_bit].any():
                        segs += 1
                        runs += runs_of(anyk[lo_bit:hi_bit])
                        single_charge_segs += int(not k[1:, lo_bit:hi_bit].any())
            for c, (lm1, hit, ok) in enumerate(cands):
                so_far[c] += int(ok[:, j0:j0 + 64].sum()) if hc[c] else 0
        with_path += int(any_taken)
        top_items.append(top)
    top_items = np.array(top_items)
    print(f"# {args.config}: first {n} spectra against {host.n_peptides} peptides, min_matched_peaks {need}; COOP_MIN_HITS {COOP_MIN_HITS}, COOP_MAX_LANES {COOP_MAX_LANES}")
    print(f"candidates restated, matched count equal to the oracle's    {agree} of {checked}")
    print(f"spectra in which the path takes a lane                      {with_path} of {n} ({100.0 * with_path / n:.0f} %)")
    print(f"lanes (candidate chunks) the path takes                     {taken} ({taken / n:.2f} per spectrum)")
    print(f"chunks with more than {COOP_MAX_LANES} heavy candidates (left to the lanes)    {crowded}")
    print(f"candidate chunks pruned in front of it                      {pruned} ({pruned / n:.1f} per spectrum)")
    print(f"bits of K1 | K2 | K3 the add loop walks                     {bits} ({bits / n:.2f} per spectrum, {bits / max(taken, 1):.1f} per lane)")
    print(f"(ion, charge) items it adds                                 {items} ({items / n:.2f} per spectrum, {items / max(taken, 1):.1f} per lane)")
    print(f"kind segments that hold a bit                               {segs} ({segs / n:.2f} per spectrum, {segs / max(taken, 1):.2f} per lane)")
    print(f"... of them matched at charge 1 only                        {single_charge_segs}")
    print(f"runs of consecutive matched ions in them                    {runs} ({runs / n:.2f} per spectrum, {bits / max(runs, 1):.2f} bits per run)")
    print(f"items per spectrum: median {np.median(top_items):.0f}, 90th percentile {np.percentile(top_items, 90):.0f}, maximum {top_items.max()}")


if __name__ == "__main__":
    main()
