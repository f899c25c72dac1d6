"""One measurement of sage_hip_protein_groups over about 1 M synthetic features, on both routes of the set cover.

    python scripts/protein_groups_bench.py [--features 1000000] [--out profiles/protein_groups_bench.json]

The world comes from the test helpers (tests/protein_groups_worlds.py): 30 000 proteins over 150 000 blocks, 2 000 of the proteins'
rings without unique peptides, so that the cover needs add_largest_to_cover picks.  Each route runs twice; the second run is
recorded (the first pays the library's one-time costs).  Routes: the default cap (edge-parallel kernels until the live edges fit
LDS, then one workgroup) and SAGE_HIP_COVER_LDS_EDGES=0 (edge-parallel kernels to the end).  There is no reference time to
compare with: no Rust toolchain here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=1_000_000)
    ap.add_argument("--proteins", type=int, default=30_000)
    ap.add_argument("--blocks", type=int, default=150_000)
    ap.add_argument("--rings", type=int, default=2_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "protein_groups_bench.json"))
    args = ap.parse_args()
    from protein_groups_worlds import build_world, draw_peptide_q, feature_table, make_blocks, ring_incidence
    from sage_amd.api import protein_groups
    rng = np.random.default_rng(2024)
    t0 = time.time()
    built = build_world(ring_incidence(rng, args.proteins, args.blocks, args.rings), make_blocks(rng, args.blocks))
    f = feature_table(built, rng, args.features)
    q = draw_peptide_q(f, rng)
    score = np.where(f["label"] == -1, rng.normal(-1.0, 1.0, len(f)), rng.normal(1.5, 2.0, len(f))).astype(np.float32)
    print(f"world: {built.host.n_peptides} peptides, {len(f)} features ({time.time() - t0:.1f} s)", flush=True)
    result = {"features": len(f), "proteins": args.proteins, "blocks": args.blocks, "peptides": int(built.host.n_peptides), "routes": {}}
    reference = None
    for name, cap in (("default_cap", None), ("bulk_only", "0")):
        if cap is None:
            os.environ.pop("SAGE_HIP_COVER_LDS_EDGES", None)
        else:
            os.environ["SAGE_HIP_COVER_LDS_EDGES"] = cap
        for _ in range(2):
            t0 = time.time()
            r = protein_groups(built.host, f, q, score)
            wall_ms = (time.time() - t0) * 1e3
        same = reference is None or (np.array_equal(r.string_id, reference.string_id) and r.strings == reference.strings and
                                     np.array_equal(r.protein_group_q, reference.protein_group_q))
        reference = reference or r
        result["routes"][name] = {"device_ms": r.device_ms, "host_graph_ms": r.host_graph_ms, "wall_ms": wall_ms,
                                  "cover_rounds": r.cover_rounds, "n_groups": r.n_groups, "n_meta_peptides": r.n_meta_peptides,
                                  "passing_protein_group": r.passing_protein_group, "same_outputs_as_first_route": bool(same)}
        print(name, json.dumps(result["routes"][name]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=2)
        fh.write("\n")


if __name__ == "__main__":
    main()
