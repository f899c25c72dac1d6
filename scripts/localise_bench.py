"""Site localisation at scale: the database and the spectra of scripts/isomer_bench.py — C3 with phospho S/T/Y,
oxidised M and N-terminal acetylation, a narrow search of --spectra synthetic spectra — then ONE Scorer.localise call over every
reported PSM that has positional isomers: its own peptide followed by the other placements.

    python scripts/localise_bench.py [--proteins 2000] [--spectra 100000] [--out profiles/localise_bench.json]

Times: HIP events on the scorer's stream (sage_hip_last_localise_timing: the whole call — uploads, both kernels, the copies back and
the host's pair selection between the kernels — and the two kernels alone) and a host clock around the call; for scale,
Scorer.score_candidates over the same lists in the same process.  One warm-up call of each, then the median of three.  No
threshold: the figures are what they are.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localise_bench.json"))
    args = ap.parse_args()
    if device_count() <= 0:
        raise SystemExit("localise_bench: no HIP device visible (there is no CPU fallback, and a CPU time would say nothing)")
    cfg = dict(CONFIGS["C3"], proteins=args.proteins, spectra=args.spectra,
               db=dict(CONFIGS["C3"]["db"], variable_mods=VARMODS, max_variable_mods=2),
               spectra_kwargs=dict(varmod_frac=0.5, varmod_residues="STYM"))
    host = build_host_db(cfg, peptides_only=True)
    groups = host.isomer_groups()
    batch, _ = workload_batch(cfg, host, 0, args.spectra)
    params = ScorerParams()
    scorer = Scorer(DeviceDatabase(host, 0), params)
    dbatch = scorer.upload(batch)
    feats, counts = scorer.score_resident(dbatch)
    feats, counts = feats.copy(), counts.copy()
    cand_off, cand_pep = cli.localisation_candidates(groups, feats, counts)
    lens = np.diff(cand_off.astype(np.int64))

    def timed(call, events):
        t = time.time()
        call()  # warm-up: code objects loaded, buffers grown, the depth scores of the counts that occur computed once
        first = (time.time() - t) * 1e3
        wall, ev = [], []
        for _ in range(3):
            t = time.time()
            call()
            wall.append((time.time() - t) * 1e3)
            ev.append(events())
        return first, float(np.median(wall)), ev

    found, scores = [], []
    loc_first, loc_wall, loc_ev = timed(lambda: found.append(scorer.localise(dbatch, feats, counts, cand_off, cand_pep)),
                                        scorer.last_localise_timing)
    _, cand_wall, cand_ev = timed(lambda: scores.append(scorer.score_candidates(dbatch, feats, counts, cand_off, cand_pep)),
                                  scorer.last_candidates_timing)
    assert all(f.tobytes() == found[0].tobytes() for f in found), "localise is not repeatable"
    cols = cli.localisation_columns(cand_off, cand_pep, found[0])
    has = cols[0] > 0
    ascore, is_best, n_site = cols[7][has], cols[8][has], cols[5][has]
    n = int(has.sum())
    out = {
        "proteins": args.proteins, "peptides": int(host.n_peptides), "spectra": int(batch.n), "psms": int(counts.sum()),
        "psms_with_isomers": n, "candidates": int(cand_off[-1]), "largest_list": int(lens.max()) if len(lens) else 0,
        "localise_call_ms": float(np.median([e[0] for e in loc_ev])), "localise_kernels_ms": float(np.median([e[1] for e in loc_ev])),
        "localise_call_ms_runs": [e[0] for e in loc_ev], "localise_kernels_ms_runs": [e[1] for e in loc_ev],
        "localise_wall_ms": loc_wall, "localise_first_call_wall_ms": loc_first,
        "score_candidates_call_ms": float(np.median([e[0] for e in cand_ev])),
        "score_candidates_kernel_ms": float(np.median([e[1] for e in cand_ev])), "score_candidates_wall_ms": cand_wall,
        "share_reported_is_best": float(is_best.mean()) if n else 0.0,
        "share_ascore_ge_13": float((ascore >= 13.0).mean()) if n else 0.0,
        "share_ascore_ge_19": float((ascore >= 19.0).mean()) if n else 0.0,
        "share_ascore_zero": float((ascore == 0.0).mean()) if n else 0.0,
        "share_without_site_determining_items": float((n_site == 0).mean()) if n else 0.0,
        "timing": "HIP events on the scorer's stream (call, kernels); host clock around the call for the *_wall_ms; median of 3 after a warm-up",
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=2)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
