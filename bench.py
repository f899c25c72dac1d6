#!/usr/bin/env python3
"""bench.py — spectra/sec of the fragment-index search-and-score path (Scorer::score over IndexedDatabase) on MI355X.

Workload = BASELINE.json configs[2] ("C3", the configuration the metric is quoted on — human tryptic narrow search; it fits
one GPU): synthetic human-sized tryptic digest (20 400 proteins, 1 missed cleavage, static C+57.0215, variable M+15.9949 and
protein-N-term +42.0106, decoys on: 4.75 M peptides, 144.7 M fragments), ±10 ppm precursor and fragment tolerance,
report_psms 1, 500 000 synthetic MS2 spectra.  --config C2 | C4 | C5 select the other BASELINE.json configurations.

One "step" = Scorer::score over this rank's share of the workload, resident in HBM: preliminary fragment matching + k-select +
rescoring + Feature assembly + the exact retry pass over tied spectra, PSM records landing in the caller's page-locked arrays
(sage_hip_score_resident: the rescoring kernels store them there themselves; one host synchronisation per step).

Multi-GPU (one process per GPU, index replicated, no collective on the data path):
  --scaling strong (default): THE workload (all 500 000 spectra of C3) is cut into N shards, rank r scores shard r; N = 1 scores all
      of it.  --shard-by mass (default): sharding.plan_mass_shards — 16 blocks of the precursor-MASS axis per rank, equal counts,
      snake order: a rank walks ~1/N of the mass-sorted index at the full batch's spectrum density (every rank generates its
      contiguous span of the synthetic run, the ranks agree on the plan from the exchanged masses and hand the spectra over through
      node-local files before the timed region).  --shard-by input: contiguous ranges of the input (round 4).  After the timed
      region the ranks' records are gathered in input order and rank 0 generates the whole run and checks the gathered result
      against its own single-GPU pass over it.  --slice K/N (one GPU): score only the shard rank K of N would get.
  --scaling weak: every rank scores its own full-size copy of the workload (different seeds).

A plain run sets up, warms up, times the steps and prints the line (its `roofline` read back from profiles/ where that holds the
configuration's bytes).  --full adds everything else: the CPU baseline and the whole-workload parity against the oracle, the live
rocprofv3 --pmc passes and the GPU algorithm's own byte counts, the sustained / concurrent / host-to-host figures and, with N > 1,
the check of the gathered records against a single-GPU pass (--no-cpu-baseline, --no-traffic, --no-extras leave parts of it out).
--dump-outputs DIR writes the records of the last timed step as DIR/<name>.npy (dump_outputs).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config C3] [--scaling strong|weak] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from sage_amd.workloads import CONFIGS, DEFAULT_CONFIG, SPECTRA_CHUNK, build_host_db, scorer_params, workload_batch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)


def host_cpu_budget():
    """How many CPUs this process may really use: the scheduler affinity mask, cut down by the cgroup CPU quota when there is
    one (cpu.max / cfs_quota_us) — os.cpu_count() is the machine's count, not ours.  Returns (cpus, details)."""
    details = {"os_cpu_count": os.cpu_count() or 1}
    try:
        details["affinity"] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        details["affinity"] = details["os_cpu_count"]
    quota = None
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: t.split()),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", lambda t: (t.strip(), None))):
        try:
            with open(path) as fh:
                q, per = parse(fh.read())
            if per is None:
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
                    per = fh.read().strip()
            details["cgroup_cpu_max"] = f"{q} {per}"
            if q not in ("max", "-1") and float(per) > 0:
                quota = float(q) / float(per)
            break
        except (OSError, ValueError):
            continue
    details["cgroup_quota_cpus"] = quota
    cpus = details["affinity"]
    if quota is not None:
        cpus = max(1, min(cpus, int(quota + 0.5)))
    return cpus, details


def _tol_str(t):
    return f"{t.kind}[{t.lo:g},{t.hi:g}]"


def same_psms(fa, ca, fb, cb):
    """Two (features[n, report_psms], counts[n]) results hold the same PSM records, byte for byte (slots beyond counts[i] are
    not part of a result: the device leaves them untouched)."""
    import numpy as np
    if not np.array_equal(ca, cb):
        return False
    valid = np.arange(fa.shape[1])[None, :] < ca[:, None]
    return fa[valid].tobytes() == fb[valid].tobytes()


DUMP_BYTES = 64_000_000  # --dump-outputs: at most this many bytes in all


def dump_outputs(path, arrays):
    """--dump-outputs: `arrays` (name -> array; one row per spectrum or PSM along axis 0, the same number of rows in each) as
    path/<name>.npy — float32 arrays as they are, every other type as float64 (exact for the integer fields).  When the rows
    would take more than DUMP_BYTES, a fixed seeded sample of them, in order; row_index.npy holds the rows written."""
    import numpy as np
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    arrays = {k: a if a.dtype == np.float32 else a.astype(np.float64) for k, a in arrays.items()}
    n = len(next(iter(arrays.values())))
    row_bytes = 8 + sum(a.itemsize * (a.size // max(n, 1)) for a in arrays.values())
    m = min(n, (DUMP_BYTES - 256 * (len(arrays) + 1)) // row_bytes)  # (each .npy file has a header of 128 bytes)
    rows = np.arange(n) if m == n else np.sort(np.random.default_rng(0).choice(n, m, replace=False))
    if m < n:
        arrays = {k: a[rows] for k, a in arrays.items()}
    arrays["row_index"] = rows.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(a))


def psm_arrays(feats, counts):
    """The PSM records a caller of the search path receives, as dump_outputs' arrays: one [spectra, report_psms] array per Feature
    field and the counts.  Slots beyond a spectrum's count are no part of the result (the device leaves them untouched): 0 here."""
    import numpy as np
    valid = np.arange(feats.shape[1])[None, :] < counts[:, None]
    out = {k: np.where(valid, feats[k], 0).astype(feats.dtype[k]) for k in feats.dtype.names if k != "pad"}
    out["counts"] = counts
    return out


def rescore_bench(args):
    """Secondary measurement: the post-search rescoring (mass-error KDE, LDA, posterior-error KDE, q-values, picked peptide /
    protein FDR) over one synthetic Feature table resident on the host, single GPU.  A "step" is one complete rescoring."""
    import numpy as np

    from sage_amd.api import Tolerance, device_count, rescore
    from sage_amd.synthetic import synthetic_features

    if device_count() <= 0:
        raise SystemExit("bench.py needs a HIP device (libsage_hip has no CPU fallback)")
    n = args.rescore_psms
    f, pk, npk, prk, npr = synthetic_features(n, seed=77)
    tol = Tolerance("ppm", -10.0, 10.0)
    for _ in range(max(1, args.warmup)):
        res = rescore(f, tol, pk, npk, prk, npr)
    wall, dev = [], []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        res = rescore(f, tol, pk, npk, prk, npr)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(res.device_ms)
    ms = float(np.mean(wall))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {k: getattr(res, k) for k in ("discriminant_score", "posterior_error", "spectrum_q",
                                                                      "peptide_q", "protein_q", "order")})
    # the Gaussian-kernel sums dominate: (mass bins + 1000 + 1000 + 1000) bins x samples evaluations of exp()
    kde_evals = 100 * n + 1000 * n + 1000 * npk + 1000 * npr
    cpu = None
    if not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib  # the CPU restatement: checker and baseline, never the product
        m = min(n, args.cpu_sample or 100_000)
        idx = np.arange(m)
        pk_s = np.unique(pk[idx], return_inverse=True)[1].astype(np.uint32)
        sel = prk[idx] != 0xFFFFFFFF
        prk_s = np.full(m, 0xFFFFFFFF, dtype=np.uint32)
        prk_s[sel] = np.unique(prk[idx][sel], return_inverse=True)[1].astype(np.uint32)
        npr_s = int(prk_s[sel].max()) + 1 if sel.any() else 0
        t0 = time.perf_counter()
        o = oracle_lib.rescore(f[idx], tol, pk_s, int(pk_s.max()) + 1, prk_s, npr_s, det=True)
        t_cpu = time.perf_counter() - t0
        g = rescore(f[idx], tol, pk_s, int(pk_s.max()) + 1, prk_s, npr_s)
        exact = all(np.array_equal(getattr(g, k), o[k]) for k in ("discriminant_score", "spectrum_q", "peptide_q", "protein_q"))
        cpu = {"value": m / t_cpu, "unit": "PSMs/s", "cores": 1, "kind": "port",
               "sample": f"the first {m} PSMs, one pass, sequential restatement (the reference parallelises the KDE sums with rayon)",
               "parity": f"lda_fitted {g.lda_fitted}=={o['lda_fitted']}, discriminants and q-values bit-identical: {exact}, "
                         f"passing {g.passing_spectrum} vs {int(o['passing'][0])}"}
    print(json.dumps({
        "metric": "PSMs/sec, post-search rescoring (LDA + KDE posterior error + q-values + picked FDR)", "value": n * 1e3 / ms,
        "unit": "PSMs/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"{n} synthetic PSMs (35 % decoys), ppm[-10,10], {npk} peptide keys, {npr} protein keys",
                   "lda_fitted": bool(res.lda_fitted), "passing_spectrum": res.passing_spectrum},
        "device_ms": float(np.mean(dev)), "kde_exp_evaluations": kde_evals,
        "kde_gexp_per_s": kde_evals / (float(np.mean(dev)) * 1e-3) / 1e9, "cpu_baseline": cpu}))


# ---- workload generation (host only; runs before this process touches the GPU) -------------------------------------------
_gen_state = {}


def _gen_chunk(c):
    cfg, host, total, seed_shift = _gen_state["cfg"], _gen_state["host"], _gen_state["total"], _gen_state["seed_shift"]
    lo, hi = _gen_state.get("span") or (0, total)
    cfg = dict(cfg, spectra_seed=cfg["spectra_seed"] + seed_shift)
    b, g = workload_batch(cfg, host, max(c * SPECTRA_CHUNK, lo), min((c + 1) * SPECTRA_CHUNK, hi), total)
    return c, b, g


_BATCH_FIELDS = ("peak_off", "masses", "intensities", "precursor_mz", "precursor_charge", "total_ion_current", "isolation_lo",
                 "isolation_hi", "scan_start_time", "inverse_ion_mobility", "file_id")


def save_batch(path, batch):
    import numpy as np
    np.savez(path, **{k: getattr(batch, k) for k in _BATCH_FIELDS if getattr(batch, k) is not None})


def load_batch(path):
    import numpy as np

    from sage_amd.api import SpectrumBatch
    z = np.load(path)
    return SpectrumBatch(*[z[k] if k in z.files else None for k in _BATCH_FIELDS])


def _whole_run_worker(conn, cfg, host, total, seed_shift, workers, path):
    """Forked by rank 0 of a strong-scaling run BEFORE it touches the GPU (a process that holds a HIP context must not fork):
    sleeps until the timed region is over, then generates the whole run for the single-GPU check and leaves it in `path`."""
    try:
        if conn.recv() != "go":
            return
        batch, _ = generate_workload(cfg, host, total, seed_shift, workers)
        save_batch(path, batch)
        conn.send("ok")
    except BaseException as e:  # noqa: BLE001
        conn.send(f"error: {e!r}")


def generate_workload(cfg, host, total, seed_shift=0, workers=None, span=None):
    """The `total` spectra of the configuration's synthetic run — or, with `span` = (lo, hi), only its spectra [lo, hi) —
    preprocessed (workloads.processed_spectra), as ONE SpectrumBatch + the global index of every kept spectrum.  The run is a
    sequence of chunks of SPECTRA_CHUNK spectra generated by forked workers (the host database is shared copy-on-write);
    chunk c depends only on (seed, c), so the result depends neither on the worker count nor on which rank generates it."""
    import multiprocessing as mp

    import numpy as np

    from sage_amd.api import SpectrumBatch
    lo, hi = span if span is not None else (0, total)
    lo, hi = max(lo, 0), min(hi, total)
    c0, c1 = (lo // SPECTRA_CHUNK, (hi + SPECTRA_CHUNK - 1) // SPECTRA_CHUNK) if hi > lo else (0, 0)
    n_chunks = max(c1 - c0, 0)
    _gen_state.update(cfg=cfg, host=host, total=total, seed_shift=seed_shift, span=(lo, hi))
    workers = workers or min(32, os.cpu_count() or 1, max(n_chunks, 1))
    _gen_chunk_warm = workload_batch(dict(cfg, spectra_seed=cfg["spectra_seed"] + seed_shift), host, 0, 1, total)  # per-database caches, before the fork
    del _gen_chunk_warm
    parts = None
    if workers > 1 and n_chunks > 1:
        try:
            # close + join, not the context manager: its terminate() sends SIGTERM to the workers, which a profiler's signal
            # handler inherited through the fork (rocprofv3 --pmc) turns into a hang
            pool = mp.get_context("fork").Pool(workers)
            try:
                parts = pool.map(_gen_chunk, range(c0, c1), chunksize=1)
            finally:
                pool.close()
                pool.join()
        except Exception as e:  # noqa: BLE001 — fall back to the serial path, say so
            print(f"bench.py: parallel workload generation failed ({e!r}); generating serially", file=sys.stderr)
            parts = None
    if parts is None:
        parts = [_gen_chunk(c) for c in range(c0, c1)]
    if not parts:
        return workload_batch(cfg, host, 0, 0, total)
    parts.sort(key=lambda p: p[0])
    bs = [p[1] for p in parts]
    off = np.zeros(sum(b.n for b in bs) + 1, dtype=np.uint64)
    pos, base = 0, 0
    for b in bs:
        off[pos + 1:pos + b.n + 1] = b.peak_off[1:] + np.uint64(base)
        pos += b.n
        base += int(b.peak_off[-1])
    cat = lambda k: None if getattr(bs[0], k) is None else np.concatenate([getattr(b, k) for b in bs])
    batch = SpectrumBatch(off, cat("masses"), cat("intensities"), cat("precursor_mz"), cat("precursor_charge"),
                          cat("total_ion_current"), cat("isolation_lo"), cat("isolation_hi"), cat("scan_start_time"),
                          cat("inverse_ion_mobility"), cat("file_id"))
    return batch, np.concatenate([p[2] for p in parts])


def shared_directory(dist, rank, coll_device):
    """A fresh directory every rank of this launch agrees on: rank 0 makes it (tempfile.mkdtemp — unique per launch, whatever
    MASTER_PORT is reused), its path goes round as a fixed-size byte tensor through ONE broadcast — a plain tensor collective
    like the barrier and the max-over-ranks, nothing that pickles.  The ranks of a bench.py launch share a node (the driver's
    contract: --nnodes=1)."""
    import torch
    buf = torch.zeros(512, dtype=torch.uint8)
    if rank == 0:
        path = tempfile.mkdtemp(prefix="sage_bench_xchg_").encode()
        assert len(path) < 512
        buf[:len(path)] = torch.tensor(list(path), dtype=torch.uint8)
    buf = buf.to(coll_device)
    dist.broadcast(buf, src=0)
    return bytes(buf.cpu().tolist()).rstrip(b"\0").decode()


def exchange_by_mass(batch, params, pep_mono, rank, world, xchg):
    """Strong scaling, --shard-by mass: every rank has generated a contiguous span of THE run; the ranks agree on
    sharding.plan_mass_shards over the whole run (per-spectrum sort mass exchanged: 8 bytes per spectrum) and
    hand each other the spectra through node-local files (the ranks of one node — the driver's contract; workload distribution
    before the timed region, not a data-path collective: a search process that reads the mzML itself, cli.py --devices, cuts its
    in-memory spectrum list instead).  `xchg`: a sharding.FileExchange over the launch's shared directory — the only thing this
    needs from torch.distributed is its barrier.  Returns (this rank's shard, the global input positions of its spectra, spectra
    in the run)."""
    import numpy as np

    from sage_amd.api import SpectrumBatch
    from sage_amd.sharding import plan_mass_shards, precursor_sort_mass
    mass = precursor_sort_mass(batch.precursor_mz, batch.precursor_charge, params)
    parts = xchg.all_gather((rank, mass), "mass")
    parts.sort(key=lambda p: p[0])
    sizes = [len(p[1]) for p in parts]
    base = int(sum(sizes[:rank]))
    n_total = int(sum(sizes))
    # (equal spectrum counts per block: a rank takes every world-th block of the mass axis, so its blocks sample every mass and
    # the shards balance without a cost model — sharding.plan_mass_shards)
    plan = plan_mass_shards(np.concatenate([p[1] for p in parts]), world)
    xdir = xchg.dir
    for j in range(world):
        mine = plan[j][(plan[j] >= base) & (plan[j] < base + batch.n)]
        sub = batch.subset(mine - base)
        np.savez(os.path.join(xdir, f"from{rank}_to{j}.npz"), index=mine,
                 **{k: getattr(sub, k) for k in _BATCH_FIELDS if getattr(sub, k) is not None})
    xchg.barrier()
    got = []
    for i in range(world):
        z = np.load(os.path.join(xdir, f"from{i}_to{rank}.npz"))
        got.append((z["index"], SpectrumBatch(*[z[k] if k in z.files else None for k in _BATCH_FIELDS])))
    xchg.barrier()
    for j in range(world):
        try:
            os.unlink(os.path.join(xdir, f"from{rank}_to{j}.npz"))
        except OSError:
            pass
    bs = [b for _, b in got]  # (sender i's pieces are ascending in the global index and the senders' spans are ordered: so is this)
    off = np.zeros(sum(b.n for b in bs) + 1, dtype=np.uint64)
    pos, pbase = 0, 0
    for b in bs:
        off[pos + 1:pos + b.n + 1] = b.peak_off[1:] + np.uint64(pbase)
        pos += b.n
        pbase += int(b.peak_off[-1])
    cat = lambda k: None if getattr(bs[0], k) is None else np.concatenate([getattr(b, k) for b in bs])  # noqa: E731
    shard = SpectrumBatch(off, *[cat(k) for k in _BATCH_FIELDS[1:]])
    index = np.concatenate([ix for ix, _ in got]).astype(np.int64)
    assert np.array_equal(index, plan[rank]), "the exchanged shard is not the planned one"
    return shard, index, n_total


# wavefronts a SIMD holds of each kernel (the compiler's table, profiles/r05_kernel_resources.txt: registers / LDS / waves_per_eu)
WAVES_PER_SIMD = {"rescore_kernel": 5, "prelim_kernel": 5, "narrow_kernel": 5, "tile_count8_kernel": 6, "tile_count_kernel": 4}


def safe_text(fn, *a):
    """A descriptive field must not take the bench line down."""
    try:
        return fn(*a)
    except Exception as e:  # noqa: BLE001
        return f"unavailable ({e!r})"


def limiters_text(dom, bound, issue, f_lines, f_alg, traffic_ps, gab, bytes_per_spec, pm, rm, n, n_wide):
    """What bounds the two phases of THIS run, in words, from this run's own figures (the text used to be a constant and went stale
    when the kernels changed)."""
    def pct(x):
        return "n/a" if x is None else f"{x:.2f}"
    kname = issue["kernel"].split("<")[0] if issue else ("rescore_kernel" if dom == "rescore" else "the dominant first-pass kernel")
    f_issue = issue["frac_issue_slots"] if issue else None
    out = [f"dominant: {kname} ({dom} phase, {max(pm, rm):.3f} of {pm + rm:.3f} ms of kernel time per step).  Against the three ceilings: "
           f"vector-instruction issue {pct(f_issue)} of its SIMDs' slots (SQ_ACTIVE_INST_VALU x wavefronts per SIMD / SQ_WAVE_CYCLES, live "
           f"rocprofv3 --pmc pass; what a scalar instruction adds: profiles/r05_valu_calibration.md), HBM line traffic {pct(f_lines)} of the "
           f"8 TB/s peak (PMC bytes), SURVEY 8(d) algorithmic bytes {pct(f_alg)} of it -> `bound` = {bound}."]
    if issue:
        out.append(f"{issue['valu_per_spectrum']:.0f} vector + {issue['salu_per_spectrum']:.0f} scalar instructions per spectrum at "
                   f"{issue['waves_per_simd']} wavefronts per SIMD: for an issue-bound kernel the lever is instructions per spectrum, not bytes.")
    ok = traffic_ps and gab and "error" not in gab
    if n_wide:
        if ok and gab.get("prelim"):
            out.append(f"Large windows: the count kernel asks for {gab['prelim'] / 1e6:.2f} MB of table words, 16-byte index cells and candidate words "
                       f"per spectrum and moves {traffic_ps.get('prelim', 0) / 1e6:.2f} MB in lines ({traffic_ps.get('prelim', 0) / gab['prelim']:.1f}x); "
                       f"SURVEY 8(d) prices the same scan at {bytes_per_spec['prelim'] / 1e6:.2f} MB (the reference's entries + probes), so here `frac` IS a "
                       f"bandwidth-like figure and issue slots and bytes are co-limiters.")
    else:
        if ok and gab.get("prelim") and pm > 0:
            out.append(f"prelim_kernel ({pm:.3f} ms) asks for {gab['prelim'] / 1e3:.1f} KB per spectrum (table words, index cells, peaks) and moves "
                       f"{traffic_ps.get('prelim', 0) / 1e3:.1f} KB in lines ({traffic_ps.get('prelim', 0) / gab['prelim']:.1f}x), "
                       f"{traffic_ps.get('prelim', 0) * n / (pm * 1e-3) / 1e9 / HBM_PEAK_GBS:.2f} of the HBM peak: neither pipe is full, it waits on "
                       f"~11 dependent round trips per spectrum (DESIGN.md 4.1).")
        out.append("by_kernel.prelim.frac above 1 and whole_path_achieved_GBs near or above the HBM peak are NOT bandwidth: 96 % of SURVEY 8(d)'s "
                   "bytes for a narrow search are the reference's binary-search probes, which a table-driven kernel never issues — an "
                   "algorithmic-work rate, not to be read against 8 TB/s.")
    return "  ".join(out)


def issue_slot_model(issue, dom):
    """The dominant kernel against the roofline that actually bounds a vector-issue-bound kernel: the fraction of its SIMDs' time the
    vector ALU was executing its instructions, from the SQ counters of a live rocprofv3 --pmc pass —
        SQ_ACTIVE_INST_VALU x (wavefronts per SIMD) / SQ_WAVE_CYCLES
    (both in quad-cycles, summed over the wavefronts; a wavefront's share of its SIMD is its resident time / the wavefronts resident
    with it).  Counted while wavefronts are resident only, so the profiler's own dispatch overhead does not enter.  Beside it the
    instruction counts per spectrum (one wavefront scores one spectrum) and the same fraction for the scalar unit."""
    if not issue or not issue.get("by_name"):
        return None
    need = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_SCA", "SQ_WAVE_CYCLES", "SQ_WAVES")
    want = ("rescore_kernel",) if dom == "rescore" else ("prelim_kernel", "tile_count")
    cands = {k: v for k, v in issue["by_name"].items() if k.startswith(want) and all(c in v for c in need)}
    if not cands:
        return None
    name = max(cands, key=lambda k: cands[k]["SQ_WAVE_CYCLES"])
    v = cands[name]
    occ = next((w for k, w in WAVES_PER_SIMD.items() if name.startswith(k)), 5)
    n = issue["n"]
    return {"kernel": name, "valu_per_spectrum": v["SQ_INSTS_VALU"] / n, "salu_per_spectrum": v["SQ_INSTS_SALU"] / n,
            "cycles_per_valu_instruction": 4.0 * v["SQ_ACTIVE_INST_VALU"] / v["SQ_INSTS_VALU"] if v["SQ_INSTS_VALU"] else None,
            "wave_cycles_per_wavefront": 4.0 * v["SQ_WAVE_CYCLES"] / v["SQ_WAVES"] if v["SQ_WAVES"] else None,
            "waves_per_simd": occ,
            "frac_issue_slots": v["SQ_ACTIVE_INST_VALU"] * occ / v["SQ_WAVE_CYCLES"] if v["SQ_WAVE_CYCLES"] else None,
            "frac_scalar_unit": v["SQ_ACTIVE_INST_SCA"] * occ / v["SQ_WAVE_CYCLES"] if v["SQ_WAVE_CYCLES"] else None,
            "source": f"rocprofv3 --pmc {' '.join(need)} in this run over {n} spectra (one dispatch per kernel and step: SAGE_HIP_WAYS=1)"}


def gpu_algorithm_bytes(dev, params, batch, n_sample=8192):
    """Bytes the GPU ALGORITHM asks memory for, per spectrum, counted by the kernels themselves in a profiling pass over a
    prefix of the workload (SAGE_HIP_PHASE_CLOCKS build of the counters, kernels.hip: DBG_*): position-table words (8 B per
    window and tile), 16-byte index cells of the flattened runs, candidate words, and for rescoring the peaks + every
    candidate's ion table.  Not lines: a 4-byte table read moves a 128-byte line (roofline.traffic has the lines)."""
    import ctypes as C

    import numpy as np

    from sage_amd import _lib as L
    from sage_amd.api import Scorer
    os.environ["SAGE_HIP_PHASE_CLOCKS"] = "1"
    try:
        sc = Scorer(dev, params)
    finally:
        del os.environ["SAGE_HIP_PHASE_CLOCKS"]
    sub = batch if batch.n <= n_sample else batch.subset(np.arange(n_sample))
    sc.score_resident(sc.upload(sub))
    out = np.zeros(32, np.uint64)
    L.check(L.load().sage_hip_debug_phase_cycles(sc._h, L.as_ptr(out, C.c_uint64)))
    sc.close()
    o = out.astype(np.float64) / sub.n
    return {"prelim": float(o[26] + o[27] + o[29] + o[30] + o[31]), "rescore": float(o[28]),
            "detail": {"narrow_table_words": float(o[26]), "narrow_index_cells_and_peaks": float(o[27]),
                       "large_window_table_words": float(o[29]), "large_window_index_cells": float(o[30]),
                       "large_window_candidate_words": float(o[31]), "rescore_peaks_candidates_ions": float(o[28])},
            "sample": sub.n}


def measure_traffic(args, kernels=("prelim", "rescore")):
    """HBM bytes per spectrum of the search kernels from rocprofv3's memory-side counters, taken NOW on this GPU in separate
    --pmc passes over a short run of this script (no kernel trace in the same pass: MI355X_MICROARCH.md §HBM, and gpurun refuses
    the combination).  FETCH_SIZE counts every 128-byte line request as 64 bytes on gfx950 — calibrated for streams, 4/8/16-byte
    gathers and short runs alike in profiles/r02_fetch_calibration.md — hence the factor 2; WRITE_SIZE is exact."""
    import glob
    import sqlite3
    if not shutil.which("rocprofv3"):
        return None, "rocprofv3 not found"
    n_spec = min(args.traffic_spectra, args.spectra or CONFIGS[args.config]["spectra"])
    tmp = tempfile.mkdtemp(prefix="sage_pmc_", dir="/tmp")
    res = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_VALU SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_WAVE_CYCLES SQ_WAVES"):
            d = os.path.join(tmp, ctr.split()[0])
            cmd = ["rocprofv3", "--pmc", *ctr.split(), "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--config",
                   args.config, "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-traffic",
                   "--no-extras"] + (["--proteins", str(args.proteins)] if args.proteins else [])
            # (a --slice run is profiled on the very shard it times: the whole run is generated and cut again in the child)
            cmd += ["--slice", args.slice, "--shard-by", args.shard_by] + (["--spectra", str(args.spectra)] if args.spectra else []) \
                if args.slice else ["--spectra", str(n_spec)]
            # (SAGE_HIP_WAYS=1: a step of this size would run as two parts — two dispatches per kernel, each over half the
            # spectra — and the largest dispatch below would no longer be the whole pass)
            env = dict(os.environ, TMPDIR="/tmp", SAGE_HIP_WAYS="1")
            p = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=args.traffic_timeout)
            if p.returncode != 0:
                return None, f"rocprofv3 --pmc {ctr} failed (rc {p.returncode}): {p.stderr[-200:]}"
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            n_scored = json.loads(line[-1])["config"]["spectra_this_rank"] if line else n_spec
            dbs = glob.glob(d + "/**/*.db", recursive=True)
            if not dbs:
                return None, "rocprofv3 wrote no database"
            con = sqlite3.connect(dbs[0])
            for name, cname, mx in con.execute("select kernel_name, counter_name, max(value) from counters_collection "
                                               "group by kernel_name, counter_name"):
                short = name.replace("sagehip::(anonymous namespace)::", "").replace("void ", "")
                key = "prelim" if (short.startswith("prelim_") or short.startswith("tile_")) else \
                    ("rescore" if short.startswith("rescore") else None)
                if key and cname in ctr.split():  # the full-pass dispatch is the largest one of each kernel (the retry pass is small)
                    res.setdefault(key, {}).setdefault(cname, 0.0)
                    res[key][cname] += mx
                    if cname.startswith("SQ_"):  # per kernel NAME as well: the issue figures belong to the one dominant kernel
                        res.setdefault("by_name", {}).setdefault(short.split("(")[0], {})[cname] = mx
            res["n"] = n_scored
    except subprocess.TimeoutExpired as e:
        tail = (e.stderr or b"")[-300:] if isinstance(e.stderr, (bytes, bytearray)) else str(e.stderr or "")[-300:]
        return None, f"traffic measurement timed out after {args.traffic_timeout} s: {tail!r}"
    except (OSError, sqlite3.Error, ValueError, KeyError) as e:
        return None, f"traffic measurement failed: {e!r}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for k in kernels:
        if k in res and "FETCH_SIZE" in res[k] and "WRITE_SIZE" in res[k]:
            out[k] = (2.0 * res[k]["FETCH_SIZE"] + res[k]["WRITE_SIZE"]) * 1024.0 / res["n"]
    if not out:
        return None, "no search kernel found in the counter tables"
    measure_traffic.issue = {"n": res["n"], "by_name": res.get("by_name", {})}
    return out, f"measured in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) over {res['n']} spectra, " \
                "(2*FETCH_SIZE + WRITE_SIZE) KiB, factor 2 per profiles/r02_fetch_calibration.md"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default=DEFAULT_CONFIG, choices=sorted(CONFIGS))
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"])
    ap.add_argument("--shard-by", default="mass", choices=["mass", "input"],
                    help="strong scaling: a rank's shard is a contiguous range of PRECURSOR MASS (sharding.plan_mass_shards, the "
                         "default: a rank walks 1/N of the mass-sorted index) or of input positions (round 4)")
    ap.add_argument("--slice", default="", metavar="K/N",
                    help="single GPU: score only the shard rank K of an N-GPU strong-scaling run would get under --shard-by (what one "
                         "GPU can say about the scaling curve: profiles/r05_shard_sizes.txt)")
    ap.add_argument("--spectra", type=int, default=0, help="override the size of the workload (smoke runs)")
    ap.add_argument("--proteins", type=int, default=0, help="override the number of proteins (smoke runs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-traffic", action="store_true", help="do not run the rocprofv3 --pmc passes (roofline.traffic from profiles/)")
    ap.add_argument("--no-extras", action="store_true", help="skip the sustained / streaming / thread-table measurements")
    ap.add_argument("--cpu-sample", type=int, default=0, help="check only this many spectra against the oracle (default: all of them)")
    ap.add_argument("--traffic-spectra", type=int, default=65536)
    ap.add_argument("--traffic-timeout", type=int, default=300)
    ap.add_argument("--rescore-psms", type=int, default=0,
                    help="measure the post-search rescoring (sage_hip_rescore, SURVEY 8f rank 4) on this many synthetic PSMs "
                         "instead of the search path; not the headline metric")
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps: CPU baseline and parity against the oracle, rocprofv3 --pmc passes, GPU algorithm "
                         "bytes, sustained / concurrent / host-to-host figures, the N > 1 check against a single-GPU pass")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the records the last timed step returned as DIR/<name>.npy (float32 / float64, at most 64 MB)")
    args = ap.parse_args()
    if not args.full:  # a plain run: the headline figure only
        args.no_cpu_baseline = args.no_traffic = args.no_extras = True
    if args.rescore_psms:
        return rescore_bench(args)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    import numpy as np
    # torch BEFORE libsage_hip: the PyTorch wheel bundles its own libamdhip64, and a process that loads the system HIP runtime
    # first (through libsage_hip.so) and torch's second ends up with two runtimes, the second of which finds no device.
    # Importing torch does not initialise the device, so the workload generator below may still fork.
    import torch  # plumbing only: device selection + the inter-rank barrier / reductions

    cfg = CONFIGS[args.config]
    total = args.spectra or cfg["spectra"]
    full_size = not args.spectra and not args.proteins
    # ---- host-side setup first (forks workers): database, the workload, this rank's shard ----
    t0 = time.time()
    need_oracle = world == 1 and not args.no_cpu_baseline
    # the reference-shaped fragment arrays are only needed by the CPU oracle leg (N = 1); the GPU index is generated on the
    # device from the peptide list either way
    host = build_host_db(cfg, args.proteins or None, peptides_only=not need_oracle)
    t_db = time.time() - t0
    t0 = time.time()
    seed_shift = rank if args.scaling == "weak" else 0
    gen_workers = max(1, min(32, int(host_cpu_budget()[0]) // world))  # (the ranks of a node share its CPUs)
    batch_all = None
    slice_info = None
    my_index = None  # strong scaling by mass: the global input positions of this rank's spectra
    if args.scaling == "strong" and world > 1:
        # Every rank generates ITS shard only: spectra [total r / N, total (r + 1) / N) of the run (whole chunks of SPECTRA_CHUNK
        # spectra except at the two ends; chunk c depends on (seed, c) only).  The synthetic run is shuffled, so
        # equal counts are equal work to ~0.5 % (sharding.plan_shards with sharding.estimate_work's weights is what a real,
        # retention-time-ordered run needs: sage_amd/cli.py).  With --full, rank 0 generates the whole run AFTER the timed region,
        # for the check of the gathered result against a single-GPU pass.
        batch, gidx = generate_workload(cfg, host, total, seed_shift, gen_workers, span=(total * rank // world, total * (rank + 1) // world))
        shards, lo, hi = None, None, None  # (positions in the whole run: known after the ranks have exchanged their counts)
        whole_run = None
        if rank == 0 and args.full:
            import multiprocessing as mp
            ctx = mp.get_context("fork")
            whole_conn, child_conn = ctx.Pipe()
            whole_path = os.path.join(tempfile.gettempdir(), f"sage_bench_whole_run_{os.getpid()}.npz")
            whole_run = ctx.Process(target=_whole_run_worker, daemon=True,
                                    args=(child_conn, cfg, host, total, seed_shift, max(1, int(host_cpu_budget()[0])), whole_path))
            whole_run.start()
    else:
        batch_all, gidx = generate_workload(cfg, host, total, seed_shift, gen_workers)
        shards, lo, hi, batch = None, 0, batch_all.n, batch_all
        if args.slice:
            from sage_amd.sharding import estimate_work, plan_mass_shards, plan_shards, precursor_sort_mass
            k_, n_ = (int(x) for x in args.slice.split("/"))
            params_ = scorer_params(cfg)
            wts = estimate_work(batch_all.peak_off, batch_all.precursor_mz, batch_all.precursor_charge, params_, host.pep_mono,
                                batch_all.isolation_lo, batch_all.isolation_hi)
            if args.shard_by == "mass":
                idx_ = plan_mass_shards(precursor_sort_mass(batch_all.precursor_mz, batch_all.precursor_charge, params_), n_)[k_]
            else:
                b_, e_ = plan_shards(batch_all.peak_off, n_, wts)[k_]
                idx_ = np.arange(b_, e_)
            batch = batch_all.subset(idx_)
            slice_info = {"slice": args.slice, "shard_by": args.shard_by, "spectra": int(batch.n),
                          "share_of_estimated_work": float(wts[idx_].sum() / wts.sum())}
    t_spec = time.time() - t0

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (libsage_hip has no CPU fallback)")
    # SAGE_BENCH_BACKEND=gloo: rehearsal of the N > 1 path on a box with fewer GPUs than ranks (ranks share devices, the
    # barrier / max-over-ranks run over gloo on CPU tensors); the driver's runs use nccl (= RCCL), one rank per GPU
    backend = os.environ.get("SAGE_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    coll_device = "cuda" if backend == "nccl" else "cpu"

    from sage_amd.api import DeviceDatabase, Scorer

    params = scorer_params(cfg)
    t0 = time.time()
    dev = DeviceDatabase(host, local_rank, build_on_device=True)  # index_build.hip: the fragment index is generated in HBM
    t_dev = time.time() - t0
    scorer = Scorer(dev, params)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # Host-side exchanges between the ranks (the mass plan and the spectra before the timed region, the ordered gather of the records
    # after it) go through files in a directory of this launch — sharding.FileExchange: the only collectives a run depends on are
    # tensor ones (this broadcast, the barrier, the max / sum over ranks).
    xchg = None
    t_exchange = 0.0
    if world > 1:
        from sage_amd.sharding import FileExchange
        xchg = FileExchange(shared_directory(dist, rank, coll_device), rank, world, barrier)
    if world > 1 and args.scaling == "strong" and args.shard_by == "mass":
        t0 = time.perf_counter()
        batch, my_index, n_run = exchange_by_mass(batch, params, host.pep_mono, rank, world, xchg)
        t_exchange = time.perf_counter() - t0
    dbatch = scorer.upload(batch)  # inputs resident in HBM before the timed region

    retry_ms = []

    # The kernels' durations come from HIP events the library records between the kernels of a step, on the scorer's own
    # streams (sage_hip_last_timing).  Every step of a full-size run; on every 4th step of a run whose steps are short (a shard of
    # an N-GPU run: <= 196 608 spectra) — the records and elapsed-time queries cost such a step ~15 us, 2 % of it
    # (profiles/r05_shard_sizes.txt) — and the averages below are over the steps that were timed.
    timing_every = 1 if batch.n > 196608 else 4

    def run(steps):
        pm, rm = [], []
        scorer.set_timing_interval(timing_every)  # (also restarts the count: step 0 of the region is a timed one)
        barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            feats, counts = scorer.score_resident(dbatch)
            if i % timing_every == 0:
                t = scorer.last_timing()
                pm.append(t["prelim_ms"])
                rm.append(t["rescore_ms"])
                retry_ms.append(t["retry_ms"])
        barrier()
        return time.perf_counter() - t0, pm, rm, feats, counts

    for _ in range(args.warmup):
        scorer.score_resident(dbatch)
    elapsed, prelim_ms, rescore_ms, feats, counts = run(args.steps)
    retry_pass_ms = float(np.mean(retry_ms)) if retry_ms else 0.0
    last_t = scorer.last_timing()
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=coll_device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        nn = torch.tensor([batch.n], dtype=torch.int64, device=coll_device)
        dist.all_reduce(nn, op=dist.ReduceOp.SUM)
        total_spectra = int(nn.item())
    else:
        total_spectra = batch.n
    ms_per_step = elapsed * 1000.0 / args.steps
    value = total_spectra * args.steps / elapsed
    feats, counts = feats.copy(), counts.copy()  # the pinned result buffers are reused by the next call

    # ---- a second, longer timed region (>= 1 s of steps) : the same number over a sustained run ----
    sustained = None
    if not args.no_extras:
        n_more = max(args.steps, int(np.ceil(1.6 / max(elapsed / args.steps, 1e-6))))  # (>= 1 s also when the longer run's steps come out faster)
        if dist is not None:
            nm = torch.tensor([n_more], dtype=torch.int64, device=coll_device)
            dist.all_reduce(nm, op=dist.ReduceOp.MAX)
            n_more = int(nm.item())
        e2, _, _, _, _ = run(n_more)
        if dist is not None:
            tt = torch.tensor([e2], dtype=torch.float64, device=coll_device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            e2 = float(tt.item())
        sustained = {"value": total_spectra * n_more / e2, "steps": n_more, "seconds": e2}

    # ---- several batches in flight: two host threads, each with its own scorer handle (sage_hip_scorer_clone: own streams and
    #      working set, same index), scoring the resident batch concurrently — how a multi-file search drives one GPU
    #      (cli.py --devices 0,0).  One thread's record download and kernel tails overlap the other's kernels.  Reported beside
    #      `value`, which stays the strictly sequential figure the roofline numbers belong to.
    concurrent = None
    if not args.no_extras:
        import threading
        n_threads = 2
        handles = [scorer] + [scorer.clone() for _ in range(n_threads - 1)]
        for h in handles[1:]:
            cf, cc = h.score_resident(dbatch)  # (allocates the clone's working set; its records must be the same)
            if not same_psms(cf, cc, feats, counts):
                raise SystemExit("bench.py: a cloned scorer handle returned different PSMs")
        per_thread = max(2, (args.steps + n_threads - 1) // n_threads)
        errors = []

        def work(h):
            try:
                for _ in range(per_thread):
                    h.score_resident(dbatch)
            except Exception as e:  # noqa: BLE001 — reported below
                errors.append(repr(e))

        barrier()
        t0 = time.perf_counter()
        ts = [threading.Thread(target=work, args=(h,)) for h in handles]
        [t.start() for t in ts]
        [t.join() for t in ts]
        barrier()
        e3 = time.perf_counter() - t0
        if errors:
            raise SystemExit(f"bench.py: concurrent scoring failed: {errors}")
        if dist is not None:
            tt = torch.tensor([e3], dtype=torch.float64, device=coll_device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            e3 = float(tt.item())
        concurrent = {"host_threads": n_threads, "steps": per_thread * n_threads, "seconds": e3,
                      "value": total_spectra * per_thread * n_threads / e3}
        del handles

    # how many ranks took part, as counted by the exchange itself (every rank reads every rank's file): in the line as n_ranks_seen
    ranks_seen = len(xchg.all_gather(int(batch.n), "alive")) if xchg is not None else 1
    # ---- strong scaling: ordered gather of the ranks' records (--dump-outputs), with --full checked against rank 0's own pass over
    #      everything ----
    sharding = None
    gathered = None
    if world > 1 and args.scaling == "strong" and (args.full or args.dump_outputs):
        from sage_amd.sharding import gather_features, gather_features_by_index
        t0 = time.perf_counter()
        sizes = xchg.all_gather(int(batch.n), "sizes")
        if my_index is not None:  # shards by precursor mass: a permutation back into input order
            gf, gc = gather_features_by_index(feats, counts, my_index, n_run, exchange=xchg)
            shards = [(0, n_run)]  # (not ranges of the input: sharding.spectra_per_rank has the counts)
        else:
            lo = int(sum(sizes[:rank]))
            hi = lo + int(batch.n)
            shards = [(int(sum(sizes[:r])), int(sum(sizes[:r + 1]))) for r in range(world)]
            gf, gc = gather_features(feats, counts, lo, exchange=xchg)  # host-side, input order, spec_index rebased
        t_gather = time.perf_counter() - t0
        gathered = gf, gc
        if rank == 0 and args.full:
            whole_conn.send("go")
            msg = whole_conn.recv()
            whole_run.join(timeout=60)
            if msg != "ok":
                raise SystemExit(f"bench.py: generating the whole run for the single-GPU check failed: {msg}")
            batch_all = load_batch(whole_path)
            os.unlink(whole_path)
            assert batch_all.n == shards[-1][1], (batch_all.n, shards)
            ref_scorer = Scorer(dev, params)
            rf, rc = ref_scorer.score(batch_all)  # the N = 1 result, through the streaming entry point
            same = same_psms(gf, gc, rf, rc)
            sharding = {"shard_by": args.shard_by if args.scaling == "strong" else None, "spectra_per_rank": [int(x) for x in sizes],
                        "shards": [list(s_) for s_ in shards], "gather_s": t_gather, "exchange_by_mass_s": t_exchange,
                        "n_ranks_seen": int(xchg.ranks_seen), "psms": int(gc.sum()), "identical_to_single_gpu": same}
            if not same:
                raise SystemExit(f"bench.py: the gathered {world}-GPU result differs from the single-GPU result")

    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, psm_arrays(*(gathered or (feats, counts))))
        n_psm = int(counts.sum())
        extras = {}
        link = None
        if not args.no_extras:
            # the host link as this box delivers it: one 256 MiB page-locked buffer each way, the ceiling of any host-to-host
            # figure below (the peaks of a step have to cross it)
            try:
                hb = torch.empty(256 << 20, dtype=torch.uint8).pin_memory()
                db_ = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
                rates = {}
                for name, src, dst in (("h2d", hb, db_), ("d2h", db_, hb)):
                    dst.copy_(src, non_blocking=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(8):
                        dst.copy_(src, non_blocking=True)
                    torch.cuda.synchronize()
                    rates[name + "_GBs"] = 8 * (256 << 20) / (time.perf_counter() - t0) / 1e9
                peak_bytes = 8.0 * float(batch.peak_off[-1]) / batch.n + 40.0  # masses + intensities + the per-spectrum arrays
                link = dict(rates, input_bytes_per_spectrum=peak_bytes,
                            host_to_host_ceiling=rates["h2d_GBs"] * 1e9 / peak_bytes)
                del hb, db_
            except Exception as e:  # noqa: BLE001 — an extra must not take the line down
                link = {"error": repr(e)}
            # host memory in, host memory out (sage_hip_score_batch: upload / score / download pipelined over chunks), on this
            # rank's share — reported beside `value`, never as `value`.  Page-locked arrays (what a caller that allocates its
            # spectrum arena with sage_hip_host_alloc hands over) and plain pageable numpy arrays.
            locked = batch.page_locked()
            host_cpu = {}
            for name, b_in in (("page_locked", locked), ("pageable", batch)):
                scorer.score(b_in)
                reps = max(3, int(0.5 / max(ms_per_step * 1e-3, 1e-4) / 4))
                c0 = time.process_time()  # (user + system CPU time of every thread of this process: the library's staging threads too)
                t0 = time.perf_counter()
                for _ in range(reps):
                    sf, sc_ = scorer.score(b_in)
                dt = time.perf_counter() - t0
                extras[name] = batch.n * reps / dt
                # what the host pays for a host-to-host call: CPU-seconds per million spectra, and how many CPUs that keeps busy
                # at the measured rate — N ranks of a node need N times that from one cgroup (VERDICT r05 task 6)
                cpu_s = time.process_time() - c0
                host_cpu[name] = {"cpu_s_per_million_spectra": cpu_s / (batch.n * reps / 1e6), "cpus_busy": cpu_s / dt}
            extras["host_cpu"] = host_cpu
            if not same_psms(sf, sc_, feats, counts):
                raise SystemExit("bench.py: the streaming entry point and the resident one disagree")
            del locked
        # ---- cpu_baseline + algorithmic bytes: the oracle (restated reference CPU path), rank 0, N = 1 only
        cpu = None
        parity = None
        bytes_per_spec = None
        cache = os.path.join(ROOT, "profiles", "algorithmic_bytes.json")
        cached = json.load(open(cache)) if os.path.exists(cache) else {}
        if world == 1 and not args.no_cpu_baseline:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import hashlib

            import oracle_lib
            from parity_utils import assert_features_equal, assert_initial_hits_equal
            ncpu, cpu_details = host_cpu_budget()
            os.environ.setdefault("OMP_PROC_BIND", "spread")
            os.environ.setdefault("OMP_PLACES", "cores")
            # ---- (1) the builds of the checker against each other on a prefix: the -O2 checker build and the -O3 performance
            #      build (same sources, strict IEEE both) must agree bit for bit, in both ln modes (1: correctly rounded through
            #      libquadmath = the product's contract, what parity is held against; 0: the platform libm = the reference's own
            #      arithmetic on this host, what is TIMED)
            n_x = min(batch.n, 2048)
            prefix = batch if n_x == batch.n else batch.subset(np.arange(n_x))
            orc = oracle_lib.OracleDb.from_product(host)
            with oracle_lib.use("fast"):
                fast = oracle_lib.OracleDb.from_product(host)
            of1, oc1, _, _ = orc.score(params, prefix, threads=0)
            with oracle_lib.LogMode(0):
                of0, oc0, _, _ = orc.score(params, prefix, threads=0)
            fast.lib.orc_set_log_mode(1)
            ff1, fc1, _, _ = fast.score(params, prefix, threads=ncpu)
            fast.lib.orc_set_log_mode(0)
            ff0, fc0, _, _ = fast.score(params, prefix, threads=ncpu)
            if not (same_psms(ff1, fc1, of1, oc1) and same_psms(ff0, fc0, of0, oc0)):
                raise SystemExit("bench.py: the performance build of the oracle differs from the checker build")
            # ---- (2) parity over the WHOLE workload of this run (VERDICT r04 task 1): every PSM of every spectrum the GPU scored
            #      in the timed region against the oracle, every field (ints and f32 bit for bit, the f64 fields through a
            #      correctly rounded ln on both sides), in slices so that the oracle's records never need more than a slice
            n_par = batch.n if not args.cpu_sample else min(batch.n, args.cpu_sample)
            fast.lib.orc_set_log_mode(1)
            t0 = time.perf_counter()
            parity_psms, step_ = 0, 65536
            for lo_ in range(0, n_par, step_):
                hi_ = min(n_par, lo_ + step_)
                sl = batch.subset(np.arange(lo_, hi_))
                of, oc, _, _ = fast.score(params, sl, threads=ncpu)
                of["spec_index"] += np.uint32(lo_)  # (a slice numbers its spectra from 0)
                parity_psms += assert_features_equal(feats[lo_:hi_], counts[lo_:hi_], of, oc, f"bench parity [{lo_}, {hi_})", exact_f64=True)
            t_parity = time.perf_counter() - t0
            fast.lib.orc_set_log_mode(0)
            # the preliminary candidate lists, heap order included (Scorer::initial_hits), on every 256th spectrum
            stride = batch.subset(np.arange(0, n_par, 256))
            hits_scorer = Scorer(dev, params)
            assert_initial_hits_equal(hits_scorer, hits_scorer.upload(stride), orc, params, stride, "bench parity, initial hits")
            hits_scorer.close()
            valid_ = np.arange(feats.shape[1])[None, :] < counts[:n_par, None]
            parity = {"spectra_checked": int(n_par), "spectra_in_workload": int(batch.n), "psms": int(parity_psms),
                      "identical": True,  # (an assertion above would have ended the run otherwise)
                      "fields": "every Feature field: integers and f32 bit for bit, f64 (hyperscore, delta_next, delta_best, poisson) "
                                "equal through a correctly rounded ln on both sides",
                      "initial_hits_checked": int(stride.n), "md5_of_gpu_records": hashlib.md5(feats[:n_par][valid_].tobytes()).hexdigest(),
                      "oracle": f"performance build of oracle/ (bit-identical to the checker build on the first {n_x} spectra in both "
                                f"ln modes), {ncpu} threads", "oracle_seconds": round(t_parity, 2)}
            # ---- (3) algorithmic bytes: the oracle's work counters on a prefix
            n_cpu = min(batch.n, cfg["cpu_sample"])
            sample = batch if n_cpu == batch.n else batch.subset(np.arange(n_cpu))
            _, _, _, work = orc.score(params, sample, threads=0, work=True)
            # ---- (4) cpu_baseline: the performance build with the platform libm, ONE sample of the workload at every thread
            #      count of the ladder (threads bound to cores; counts beyond the CPUs this process is allowed only get throttled)
            n_time = min(batch.n, cfg.get("cpu_time_sample", cfg["cpu_sample"]))
            tsample = batch if n_time == batch.n else batch.subset(np.arange(n_time))
            fast.score(params, tsample, threads=ncpu)  # warm-up (page in the index)
            table = {}
            ladder = sorted({t for t in (1, 2, 4, 8, 16, 32, 64, 128, 256) if t <= ncpu} | {ncpu})
            if args.no_extras:
                ladder = [ncpu]
            for th in ladder:
                _, _, ms, _ = fast.score(params, tsample, threads=th)
                table[str(th)] = {"spectra_per_s": tsample.n * 1000.0 / ms, "spectra": tsample.n, "seconds": ms / 1e3}  # runner.rs:327-330
            best = max(table, key=lambda k: table[k]["spectra_per_s"])
            cpu = {"value": table[best]["spectra_per_s"], "unit": "spectra/s", "cores": int(best), "kind": "port",
                   "host_cpus_allowed": ncpu, "host_cpu_details": cpu_details,
                   "sample": f"the first {tsample.n} of the {batch.n} spectra of the workload — the SAME sample at every thread count "
                             f"of threads_table, one pass each after one warm-up, OpenMP dynamic schedule, threads bound to cores "
                             f"(OMP_PROC_BIND=spread), performance build of the restated reference CPU path (oracle/Makefile FASTFLAGS, "
                             f"platform libm; not Sage itself — no Rust toolchain here); value = the best thread count up to the "
                             f"{ncpu} CPUs this process may use",
                   "threads_table": table,
                   "parity": f"{parity_psms} PSMs of {n_par} spectra identical to the GPU result (see the line's `parity` object)"}
            rescore_bytes = 4 * work["rescored"] + 5 * work["rescored_residues"] + 64 * work["reported"]
            bytes_per_spec = {"total": work["algorithmic_bytes"] / sample.n,
                              "prelim": (work["algorithmic_bytes"] - rescore_bytes) / sample.n,
                              "rescore": rescore_bytes / sample.n}
            if full_size:
                try:
                    cached[args.config] = {"bytes_per_spectrum": bytes_per_spec, "work": work, "n_spectra": sample.n}
                    os.makedirs(os.path.dirname(cache), exist_ok=True)
                    json.dump(cached, open(cache, "w"), indent=1)
                except OSError:
                    pass
        elif args.config in cached:
            bytes_per_spec = cached[args.config]["bytes_per_spectrum"]

        pm, rm = float(np.mean(prelim_ms)), float(np.mean(rescore_ms))
        dom = "prelim" if pm >= rm else "rescore"
        roof = None
        if bytes_per_spec:
            dom_ms = max(pm, rm)
            achieved = bytes_per_spec[dom] * batch.n / (dom_ms * 1e-3) / 1e9
            traffic_ps, source = None, None
            if world == 1 and not args.no_traffic:
                traffic_ps, source = measure_traffic(args)
            if traffic_ps is None:
                why = source
                tpath = os.path.join(ROOT, "profiles", "traffic.json")
                tj = json.load(open(tpath)).get(args.config, {}) if os.path.exists(tpath) else {}
                if tj.get(dom + "_bytes_per_spectrum"):
                    traffic_ps = {k: tj[k + "_bytes_per_spectrum"] for k in ("prelim", "rescore") if tj.get(k + "_bytes_per_spectrum")}
                    source = f"read back from profiles/traffic.json ({tj.get('source', '?')})" + (f"; not measured now: {why}" if why else "")
                else:
                    source = f"unavailable ({why})" if why else "unavailable"
            traffic = traffic_ps[dom] * batch.n if traffic_ps and dom in traffic_ps else None
            gab = None
            if not args.no_extras:
                try:
                    gab = gpu_algorithm_bytes(dev, params, batch)
                except Exception as e:  # noqa: BLE001 — a profiling extra must not take the line down
                    gab = {"error": repr(e)}
            issue = issue_slot_model(getattr(measure_traffic, "issue", None), dom)
            # which ceiling the dominant kernel sits under: its share of the vector-issue slots (a live counter pass) against its share of
            # the HBM peak in line traffic — whichever is nearer 1.  `achieved` / `peak` / `frac` / `traffic` stay the HBM figures the
            # contract names (SURVEY 8(d) bytes, PMC bytes); `frac_issue_slots` is the fraction of the ceiling `bound` names when it
            # says "valu_issue" (VERDICT r05 task 7: the line said "hbm" for a kernel its own text called issue-bound).
            f_issue = issue["frac_issue_slots"] if issue else None
            f_lines = None if traffic is None else traffic / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
            bound = "valu_issue" if f_issue is not None and (f_lines is None or f_issue > f_lines) else "hbm"
            roof = {"bound": bound, "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": source,
                    # the second fraction: bytes that actually crossed the HBM interface (PMC) over the same kernel time
                    "achieved_traffic": None if traffic is None else traffic / (dom_ms * 1e-3) / 1e9,
                    "frac_traffic": None if traffic is None else traffic / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "traffic_bytes_per_spectrum": traffic_ps,
                    # the third figure: what the GPU algorithm itself requests (table words, index cells, candidates, ions)
                    "gpu_algorithm_bytes_per_spectrum": gab,
                    "frac_gpu_algorithm": None if not gab or "error" in gab else gab[dom] * batch.n / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    # the fourth figure, and for an issue-bound kernel the one that IS its roofline (VERDICT r04 task 7): the
                    # instruction-issue slots the kernel's wavefronts take of the slots its SIMDs had (issue_slot_model)
                    "issue": issue, "frac_issue_slots": None if not issue else issue["frac_issue_slots"],
                    "kernel_ms": {"prelim": pm, "rescore": rm, "of_which_exact_retry_pass": retry_pass_ms,
                                  "timed_steps": f"every {timing_every}. step of the timed region" if timing_every > 1 else "every step of the timed region"},
                    # both phases, each against the HBM roofline with the same three byte counts (the top-level fields repeat
                    # the entry of the phase that takes longer)
                    "by_kernel": {k: {"ms": ms_k,
                                      "frac": bytes_per_spec[k] * batch.n / (ms_k * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                      "frac_traffic": None if not traffic_ps or k not in traffic_ps else
                                      traffic_ps[k] * batch.n / (ms_k * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                      "frac_gpu_algorithm": None if not gab or "error" in gab else
                                      gab[k] * batch.n / (ms_k * 1e-3) / 1e9 / HBM_PEAK_GBS}
                                  for k, ms_k in (("prelim", pm), ("rescore", rm)) if ms_k > 0},
                    "limiters": safe_text(limiters_text, dom, bound, issue, f_lines, achieved / HBM_PEAK_GBS, traffic_ps, gab, bytes_per_spec, pm, rm,
                                          batch.n, last_t["n_wide"]),
                    "algorithmic_bytes_per_spectrum": bytes_per_spec,
                    "whole_path_achieved_GBs": bytes_per_spec["total"] * batch.n / ((pm + rm) * 1e-3) / 1e9,
                    "routing": {"spectra": batch.n, "large_window_kernel": last_t["n_wide"],
                                # equal hyperscores at the reported rank: settled by the tie kernels from the window counts the first
                                # pass keeps (one reported PSM), the rest through the exact retry pass
                                "ties_settled_from_stored_counts": last_t["n_tied"],
                                "exact_retry_for_tied_hyperscores": last_t["n_retry"], "launches_per_step": last_t["n_launches"],
                                # > 1: the step ran as that many parts on their own streams (steps of up to 196 608 spectra without
                                # large windows) and kernel_ms are sums over launches that overlap in time
                                "parts_per_step": last_t["n_ways"]},
                    "note": "achieved / frac: SURVEY 8(d) algorithmic bytes of the reference's algorithm (binary-search probes "
                            "at 4-8 B each + scanned entries) over the dominant phase's kernel time (HIP events on the scorer's "
                            "stream). achieved_traffic / frac_traffic: the bytes the GPU kernels really moved (128-byte lines; a "
                            "4-byte table read costs a line) over the same time. prelim = fragment matching + k-select kernels."}
        out = {
            "metric": cfg["metric"],
            "value": value, "unit": "spectra/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": cfg["name"] + f", {total} spectra" + ("" if args.scaling == "strong" else " per GPU"),
                       "spectra_total": total_spectra, "spectra_this_rank": batch.n, "peptides": host.n_peptides,
                       "fragments": host.n_fragments if host.has_fragments else None, "precursor_tol": _tol_str(params.precursor_tol),
                       "fragment_tol": _tol_str(params.fragment_tol), "report_psms": params.report_psms,
                       "chimera": params.chimera, "wide_window": params.wide_window,
                       "parallelism": f"spectra sharded x{world} ({args.scaling}" + (f", contiguous in precursor {args.shard_by}" if world > 1 and args.scaling == "strong" else "") + "), index replicated, no collective on the data path",
                       "slice": slice_info,
                       "psms_per_step_rank0": n_psm,
                       "setup_s": {("db_build_host_incl_fragments_for_the_oracle" if need_oracle else "db_build_host_peptides"): round(t_db, 2),
                                   "spectra": round(t_spec, 2),
                                   "index_build_on_device": round(t_dev, 2)},
                       "index_device_bytes": dev.device_bytes},
            "roofline": roof, "cpu_baseline": cpu,
            "parity": parity,  # the whole workload of this run against the oracle (N = 1 only)
            "sustained": sustained,
            "concurrent": concurrent,  # two scorer handles / host threads on the same GPU (see above)
            "host_to_host_value": extras or None,  # PCIe-inclusive: sage_hip_score_batch, this rank's share
            "host_link": link,  # measured link rates and the host-to-host ceiling they imply for this workload
            "pcie_inclusive_value": extras.get("page_locked") if extras else None,
            # the like-for-like figure against the reference's own clock (runner.rs:327-330 starts and ends in host memory), as a
            # fraction of what the measured link allows for this workload's input bytes
            "host_to_host_frac_of_link": (extras["page_locked"] / link["host_to_host_ceiling"]
                                          if extras and link and link.get("host_to_host_ceiling") else None),
            "sharding": sharding,
            "n_ranks_seen": ranks_seen,
        }
        if cpu:
            out["speedup_vs_cpu_baseline"] = value / cpu["value"]
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        if rank == 0 and xchg is not None:
            import shutil
            shutil.rmtree(xchg.dir, ignore_errors=True)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
