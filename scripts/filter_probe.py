"""What the peak-bitmap filter of rescore_kernel costs per spectrum, and what dealing its ions to all 64 lanes saves,
from the oracle alone — no GPU:

    python scripts/filter_probe.py [--config C3] [--spectra 800] [--proteins 0]  > profiles/rNN_filter_probe.txt
    python scripts/filter_probe.py --gpu ...     the device's own counters over the same spectra instead (needs a GPU)

For each of the first spectra of a bench.py configuration: the preliminary list (OracleDb.initial_hits), every valid candidate's
ion count (n_kinds x (length - 1)) and the fragment charges tested, nfz = min(z - 1, 3) (charges above 3 are not filtered).  Per
64-ion chunk the per-lane filter runs ceil(longest candidate's ions in the chunk / 4) trips of 4 ions; ions dealt in groups of g
cost ceil(sum over candidates of ceil(ions in the chunk / g) / 64) trips of g ions.  The table's unit is one 4-ion trip of the
wavefront, counted once per fragment charge tested (a trip of 8 ions counts 2).  Below the table: the same spectra through the
wave-uniform choice the kernel makes (core.h: flat_route_wins) in the units of the profiling instance's counters
(sage_hip_debug_filter_counters), which --gpu prints for the device."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLAT_MARGIN = 1  # core.h: SAGE_FLAT_MARGIN
FLAT_EXTRA_BYTES = 384  # kernels.hip


def flat_fits(octets, charges, pcap):
    """core.h: flat_area_bytes(octets, charges) <= kernels.hip: rescore_flat_bytes(pcap) — the chunk's item bytes fit the area"""
    return ((octets + 3) & ~3) * charges + 12 <= ((2 * pcap + 7) & ~7) + FLAT_EXTRA_BYTES
BANDS = ((1, 16), (17, 32), (33, 49), (50, 50))


def candidates(orc, params, batch, i, ions_of):
    """(ions, precursor charge) of every valid candidate of spectrum i's preliminary list"""
    packed, _, _ = orc.initial_hits(params, batch, i)
    out = []
    for word in packed:
        word = int(word)
        pep, z = (word >> 16) & 0xFFFFFFFF, (word >> 8) & 0xFF
        if pep == 0xFFFFFFFF or (word >> 48) == 0:
            continue
        out.append((int(ions_of[pep]), z))
    return out


def gpu_counters(args, host, params, batch):
    import ctypes as C

    from sage_amd import _lib as L
    from sage_amd.api import DeviceDatabase, Scorer
    os.environ["SAGE_HIP_PHASE_CLOCKS"] = "1"
    scorer = Scorer(DeviceDatabase(host, 0), params)
    del os.environ["SAGE_HIP_PHASE_CLOCKS"]
    _, counts = scorer.score_resident(scorer.upload(batch))
    out = np.zeros(4, np.uint64)
    L.check(L.load().sage_hip_debug_filter_counters(scorer._h, L.as_ptr(out, C.c_uint64)))
    t = scorer.last_timing()
    n = batch.n
    print(f"# {args.config}: first {n} spectra on the device (profiling instance), {int(counts.sum())} PSMs, n_retry {t['n_retry']}, n_tied {t['n_tied']}"
          f" (a spectrum of the retry pass is filtered twice)")
    print(f"64-ion chunks that took the flat route          {int(out[0])}")
    print(f"their trips of 8 ions                           {int(out[1])} ({out[1] / n:.2f} per spectrum)")
    print(f"trips of 4 ions the per-lane filter would make  {int(out[2])} ({out[2] / n:.2f} per spectrum)")
    print(f"trips of 4 ions of the chunks left per-lane     {int(out[3])} ({out[3] / n:.2f} per spectrum)")
    print(f"4-ion trips per spectrum: {(2 * out[1] + out[3]) / n:.2f} against {(out[2] + out[3]) / n:.2f} per-lane")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--spectra", type=int, default=800)
    ap.add_argument("--proteins", type=int, default=0)
    ap.add_argument("--gpu", action="store_true", help="score the same spectra on device 0 and print the profiling instance's filter counters")
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
    n_kinds = len(host.ion_kinds)
    lens = np.diff(host.seq_off.astype(np.int64))
    ions_of = n_kinds * np.maximum(lens - 1, 0)
    rows = {b: np.zeros(4) for b in BANDS}  # spectra, now, groups of 8, groups of 4
    dev = np.zeros(4)                        # the device counters' units: flat chunks, flat trips, would, per-lane trips
    none_valid = chunks = no_room = 0
    pcap = int(np.diff(batch.peak_off.astype(np.int64)).max())  # the batch's peak capacity: what the kernel's LDS is carved for
    for i in range(batch.n):
        cands = candidates(orc, params, batch, i, ions_of)
        if not cands:
            none_valid += 1
            continue
        nfz = min(max(z for _, z in cands) - 1, 3)
        now = g8 = g4 = 0
        for j0 in range(0, max(n for n, _ in cands), 64):
            here = np.array([min(max(n - j0, 0), 64) for n, z in cands if z - 1 <= 3])  # (unfiltered lanes own no items)
            everyone = np.array([min(max(n - j0, 0), 64) for n, _ in cands])
            would = int(-(-everyone.max() // 4))
            now += would
            o8, o4 = int((-(-here // 8)).sum()), int((-(-here // 4)).sum())
            g8 += 2 * -(-o8 // 64)
            g4 += -(-o4 // 64)
            longest = int((-(-here // 8)).max()) if len(here) else 0
            charges = 1 + any(z - 1 >= 2 for _, z in cands) + any(z - 1 >= 3 for _, z in cands)  # (any_fz2, any_fz3)
            wins = o8 and -(-o8 // 64) + FLAT_MARGIN < longest
            if wins and not flat_fits(o8, charges, pcap):
                no_room += 1
            if wins and flat_fits(o8, charges, pcap):
                dev += (1, -(-o8 // 64), would, 0)
            else:
                dev += (0, 0, 0, would)
            chunks += 1
        band = next(b for b in BANDS if b[0] <= len(cands) <= b[1])
        rows[band] += (1, now * nfz, g8 * nfz, g4 * nfz)
    n = batch.n
    print(f"# {args.config}: first {n} spectra against {host.n_peptides} peptides; 4-ion trips of the wavefront per spectrum, once per fragment charge tested")
    print(f"{'valid candidates':<18}{'share of spectra':>18}{'now':>8}{'groups of 8':>14}{'groups of 4':>14}")
    tot = np.zeros(4)
    for (a, b), r in rows.items():
        tot += r
        k = max(r[0], 1)
        print(f"{(str(a) if a == b else f'{a}-{b}'):<18}{r[0] / n:>18.2f}{r[1] / k:>8.1f}{r[2] / k:>14.1f}{r[3] / k:>14.1f}")
    k = max(tot[0], 1)
    print(f"{'all':<18}{tot[0] / n:>18.2f}{tot[1] / k:>8.1f}{tot[2] / k:>11.1f} ({100 * tot[2] / max(tot[1], 1):.0f} %)"
          f"{tot[3] / k:>8.1f} ({100 * tot[3] / max(tot[1], 1):.0f} %)")
    print(f"spectra with no valid candidate: {none_valid} of {n}")
    print(f"# the kernel's choice (flat when ceil(octets / 64) + {FLAT_MARGIN} < the longest lane's octets and the item bytes fit the area: "
          f"{((2 * pcap + 7) & ~7) + FLAT_EXTRA_BYTES} bytes at {pcap} peaks), in the device counters' units, first pass only")
    print(f"64-ion chunks that take the flat route          {int(dev[0])} of {chunks} ({no_room} more would win, but their bytes do not fit)")
    print(f"their trips of 8 ions                           {int(dev[1])} ({dev[1] / n:.2f} per spectrum)")
    print(f"trips of 4 ions the per-lane filter would make  {int(dev[2])} ({dev[2] / n:.2f} per spectrum)")
    print(f"trips of 4 ions of the chunks left per-lane     {int(dev[3])} ({dev[3] / n:.2f} per spectrum)")
    print(f"4-ion trips per spectrum: {(2 * dev[1] + dev[3]) / n:.2f} against {(dev[2] + dev[3]) / n:.2f} per-lane")


if __name__ == "__main__":
    main()
