"""Isomer scoring at scale: a C3-style database with phospho S/T/Y, oxidised M and N-terminal acetylation, so that
most PSMs have positional isomers; a narrow search of --spectra synthetic spectra, then ONE Scorer.score_candidates call over every
reported PSM's isomers.

    python scripts/isomer_bench.py [--proteins 2000] [--spectra 100000] [--out profiles/isomers_bench.json]

Times: HIP events on the scorer's stream (sage_hip_last_candidates_timing: the whole call, and the kernel alone) and a host clock
around the call, which ends in a stream synchronise; for scale, the host clock around sage_hip_annotate_resident over the same PSMs
in the same process.  One warm-up call of each, then the median of three.  No threshold: the figures are what they are.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sage_amd import cli  # noqa: E402
from sage_amd.api import DeviceDatabase, Scorer, ScorerParams, device_count  # noqa: E402
from sage_amd.workloads import CONFIGS, build_host_db, workload_batch  # noqa: E402

VARMODS = {"M": [15.9949], "S": [79.9663], "T": [79.9663], "Y": [79.9663], "[": [42.010565]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=2000)
    ap.add_argument("--spectra", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isomers_bench.json"))
    args = ap.parse_args()
    if device_count() <= 0:
        raise SystemExit("isomer_bench: no HIP device visible (there is no CPU fallback, and a CPU time would say nothing)")
    cfg = dict(CONFIGS["C3"], proteins=args.proteins, spectra=args.spectra,
               db=dict(CONFIGS["C3"]["db"], variable_mods=VARMODS, max_variable_mods=2),
               spectra_kwargs=dict(varmod_frac=0.5, varmod_residues="STYM"))
    t0 = time.time()
    host = build_host_db(cfg, peptides_only=True)
    t1 = time.time()
    groups = host.isomer_groups()
    t2 = time.time()
    group_of, group_off, members = groups
    sizes = np.diff(group_off.astype(np.int64))
    batch, _ = workload_batch(cfg, host, 0, args.spectra)
    params = ScorerParams()
    scorer = Scorer(DeviceDatabase(host, 0), params)
    dbatch = scorer.upload(batch)
    feats, counts = scorer.score_resident(dbatch)
    feats, counts = feats.copy(), counts.copy()
    cand_off, cand_pep = cli.isomer_candidates(groups, feats, counts)
    lens = np.diff(cand_off.astype(np.int64))

    def timed(call, events=None):
        call()  # warm-up: code objects loaded, scratch buffers grown
        wall, ev = [], []
        for _ in range(3):
            t = time.time()
            call()
            wall.append((time.time() - t) * 1e3)
            if events:
                ev.append(events())
        return float(np.median(wall)), ev

    scores = []
    cand_wall, ev = timed(lambda: scores.append(scorer.score_candidates(dbatch, feats, counts, cand_off, cand_pep)),
                          scorer.last_candidates_timing)
    ann_wall, _ = timed(lambda: scorer.annotate(dbatch, feats, counts))
    assert all(s.tobytes() == scores[0].tobytes() for s in scores), "score_candidates is not repeatable"
    n_iso, _, best_h, _ = cli.best_isomers(cand_off, cand_pep, scores[0])
    has = n_iso > 0
    delta = feats["hyperscore"].reshape(-1)[has] - best_h[has]
    out = {
        "proteins": args.proteins, "peptides": int(host.n_peptides), "peptides_in_groups": int((group_of != 0xFFFFFFFF).sum()),
        "groups": int(len(sizes)), "largest_group": int(sizes.max()) if len(sizes) else 0,
        "host_digest_ms": (t1 - t0) * 1e3, "isomer_groups_ms": (t2 - t1) * 1e3,
        "spectra": int(batch.n), "psms": int(counts.sum()), "psms_with_isomers": int(has.sum()),
        "spectra_with_candidates": int((lens.reshape(batch.n, -1).sum(axis=1) > 0).sum()),
        "candidates_scored": int(cand_off[-1]), "largest_list": int(lens.max()) if len(lens) else 0,
        "score_candidates_call_ms": float(np.median([e[0] for e in ev])), "score_candidates_kernel_ms": float(np.median([e[1] for e in ev])),
        "score_candidates_call_ms_runs": [e[0] for e in ev], "score_candidates_kernel_ms_runs": [e[1] for e in ev],
        "score_candidates_wall_ms": cand_wall, "annotate_wall_ms": ann_wall, "annotated_fragments": int(feats["matched_peaks"].reshape(-1)[
            (np.arange(params.report_psms)[None, :] < counts[:, None]).reshape(-1)].sum()),
        "psms_with_delta_isomer_zero": int((delta == 0.0).sum()), "psms_with_delta_isomer_negative": int((delta < 0.0).sum()),
        "timing": "HIP events on the scorer's stream (call, kernel); host clock around the call for the *_wall_ms; median of 3 after a warm-up",
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=2)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
