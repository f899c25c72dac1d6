"""A plain-Python reading of the reference's protein grouping and picked protein-group competition keys — dicts, tuples and
sorted lists, written from crates/sage/src/protein_grouping.rs:59-386 and fdr.rs:192-226, independent of the product's code.

A world is what the reference reads of its IndexedDatabase: for every peptide index its protein names in stored order and its
decoy flag, plus `decoy_tag` and `generate_decoys`.  TEST INFRASTRUCTURE (no test in this file).
"""
import numpy as np


class World:
    def __init__(self, proteins_of, decoy, decoy_tag="rev_", generate_decoys=True):
        self.proteins_of = proteins_of        # list (by peptide index) of lists of names, stored order
        self.decoy = [bool(d) for d in decoy]  # by peptide index
        self.decoy_tag = decoy_tag
        self.generate_decoys = generate_decoys

    def fallback(self, pep):
        """Peptide::proteins (peptide.rs:81-97) and Peptide.proteins.len()"""
        tag = self.decoy_tag if (self.decoy[pep] and self.generate_decoys) else ""
        return ";".join(tag + name for name in self.proteins_of[pep]), len(self.proteins_of[pep])


def into_cover(edges, n_left, n_right):
    """BipartiteGraph::new(edges, n_left, n_right).into_cover() (:75-156), sequentially.  Returns (cover, add_largest picks)."""
    edges = list(edges)
    left_degree, right_degree = [0] * n_left, [0] * n_right
    for l, r in edges:
        left_degree[l] += 1
        right_degree[r] += 1
    original = list(left_degree)
    left_cover, right_cover = [False] * n_left, [False] * n_right
    picks = 0
    while edges:
        prev = 0
        while prev != len(edges):  # trim
            prev = len(edges)
            for l, r in edges:
                if right_degree[r] == 1:
                    left_cover[l] = True
            kept = []
            for l, r in edges:
                if left_cover[l]:
                    right_cover[r] = True
                    left_degree[l] -= 1
                    right_degree[r] -= 1
                else:
                    kept.append((l, r))
            edges = kept
            kept = []
            for l, r in edges:
                if right_cover[r]:
                    left_degree[l] -= 1
                    right_degree[r] -= 1
                else:
                    kept.append((l, r))
            edges = kept
        if edges:  # add_largest_to_cover: Iterator::max_by_key returns the LAST maximum
            best, best_key = None, None
            for i in range(n_left):
                key = (left_degree[i], original[i])
                if best_key is None or key >= best_key:
                    best, best_key = i, key
            left_cover[best] = True
            picks += 1
    return left_cover, picks


def build_graph(world, selected):
    """ProteinGrouper::build (:171-231) for the set `selected` of peptide indices.  Returns a dict:
    proteins  [(name, decoy)] in ProteinIx order        metas     sorted list of the distinct ProteinIx tuples
    groups    [tuple of ProteinIx, ascending]            evidence  [tuple of meta-peptide indices] per group
    edges     [(group, meta-peptide)]"""
    index = {}
    metas = set()
    for pep in sorted(set(selected)):
        ids = []
        for name in world.proteins_of[pep]:
            key = (name, world.decoy[pep])
            if key not in index:
                index[key] = len(index)
            ids.append(index[key])
        metas.add(tuple(sorted(ids)))
    metas = sorted(metas)
    prot_to_metas = {}
    for i, meta in enumerate(metas):
        for ix in meta:
            prot_to_metas.setdefault(ix, []).append(i)
    evidence_to_group = {}
    for ix, ev in prot_to_metas.items():
        evidence_to_group.setdefault(tuple(ev), []).append(ix)
    groups, evidence, edges = [], [], []
    for g, (ev, members) in enumerate(sorted(evidence_to_group.items())):
        groups.append(tuple(sorted(members)))
        evidence.append(ev)
        edges += [(g, m) for m in ev]
    proteins = [k for k, _ in sorted(index.items(), key=lambda kv: kv[1])]
    return dict(proteins=proteins, metas=metas, groups=groups, evidence=evidence, edges=edges)


def _format_group(world, graph, g):
    names = []
    for ix in graph["groups"][g]:
        name, decoy = graph["proteins"][ix]
        names.append(world.decoy_tag + name if (decoy and world.generate_decoys) else name)
    return "/".join(sorted(names))


def _annotate(world, selected, assigned, peptides):
    """annotate_features (:341-386) per distinct peptide: fills `assigned[pep] = (string, count)` where it is still absent.
    Returns (graph, add_largest picks)."""
    graph = build_graph(world, selected)
    cover, picks = into_cover(graph["edges"], len(graph["groups"]), len(graph["metas"]))
    protein_to_groups = {}
    for g, inside in enumerate(cover):
        if inside:
            for ix in graph["groups"][g]:
                protein_to_groups.setdefault(graph["proteins"][ix], []).append(g)
    for pep in peptides:
        if pep in assigned:
            continue
        group_set = set()
        for name in world.proteins_of[pep]:
            group_set.update(protein_to_groups.get((name, world.decoy[pep]), ()))
        if not group_set:
            continue
        s = ";".join(sorted(_format_group(world, graph, g) for g in group_set))
        assigned[pep] = (s, s.count(";") + 1)
    return graph, picks


def generate_protein_groups(world, label, peptide_idx, peptide_q, protein_grouping=True, peptide_fdr=0.01):
    """generate_protein_groups (:312-339) with Some(peptide_fdr).  Returns a dict: strings [n], num [n] (per feature), and of
    the passes: n_groups / n_meta_peptides of the last one, picks summed, selected / edges = the sizes of each pass's selection and
    edge list."""
    label = np.asarray(label)
    peptide_idx = [int(p) for p in peptide_idx]
    q = np.asarray(peptide_q, dtype=np.float32)
    peptides = sorted(set(peptide_idx))
    assigned = {}
    stats = dict(n_groups=0, n_meta_peptides=0, picks=0, selected=[], edges=[])
    if protein_grouping:
        with np.errstate(invalid="ignore"):
            t1 = np.float32(peptide_fdr)
            t1 = t1 if np.isnan(t1) else min(max(t1, np.float32(0.0)), np.float32(1.0))  # f32::clamp keeps a NaN
            for t in (t1, np.float32(1.0)):
                chosen = {p for p, l, x in zip(peptide_idx, label, q) if l != -1 and x < t}
                graph, picks = _annotate(world, chosen, assigned, peptides)
                stats["n_groups"], stats["n_meta_peptides"] = len(graph["groups"]), len(graph["metas"])
                stats["picks"] += picks
                stats["selected"].append(len(chosen))
                stats["edges"].append(len(graph["edges"]))
    for pep in peptides:
        if pep not in assigned:
            assigned[pep] = world.fallback(pep)
    return dict(strings=[assigned[p][0] for p in peptide_idx], num=np.array([assigned[p][1] for p in peptide_idx], dtype=np.uint32),
                **stats)


NO_KEY = 0xFFFFFFFF


def competition_keys(strings, num):
    """picked_protein_group's map keys (fdr.rs:196-213): features with num_protein_groups == 1, keyed by the string; dense ids in
    order of first appearance, NO_KEY for the features that take no part.  Returns (keys[n], n_keys)."""
    ids = {}
    keys = np.full(len(strings), NO_KEY, dtype=np.uint32)
    for i, (s, k) in enumerate(zip(strings, num)):
        if int(k) == 1:
            keys[i] = ids.setdefault(s, len(ids))
    return keys, len(ids)
