// groups.cpp — the host half of protein grouping (crates/sage/src/protein_grouping.rs:159-231, ProteinGrouper::build): protein
// numbering, meta-peptides, groups and the edge list of the set cover, from the ascending list of selected peptides.  Strings and
// orderings of vectors live here; the device (protein_groups.hip) sees the dense ids this file hands out.
#include <algorithm>
#include <numeric>
#include <unordered_map>

#include "host_db.hpp"

namespace sagehip {

NameIndex::NameIndex(const HostDb& db) : of_protein(db.protein_names.size()) {
    std::unordered_map<std::string, uint32_t> ids;
    ids.reserve(db.protein_names.size());
    for (size_t i = 0; i < db.protein_names.size(); ++i)
        of_protein[i] = ids.emplace(db.protein_names[i], (uint32_t)ids.size()).first->second;
    n_names = (uint32_t)ids.size();
}

namespace {

// lexicographic order of rows [off[a], off[a + 1]) of `v`: a shorter prefix first (Vec<T>::cmp)
struct RowLess {
    const std::vector<uint64_t>& off;
    const std::vector<uint32_t>& v;
    int cmp(uint32_t a, uint32_t b) const {
        const uint32_t *pa = v.data() + off[a], *ea = v.data() + off[a + 1], *pb = v.data() + off[b], *eb = v.data() + off[b + 1];
        for (; pa != ea && pb != eb; ++pa, ++pb)
            if (*pa != *pb) return *pa < *pb ? -1 : 1;
        return pa == ea ? (pb == eb ? 0 : -1) : 1;
    }
    bool operator()(uint32_t a, uint32_t b) const { return cmp(a, b) < 0; }
};

}  // namespace

void build_group_graph(const HostDb& db, const NameIndex& names, const uint32_t* peptides, uint64_t n, GroupGraph& out) {
    out = GroupGraph{};
    // :176-192: ProteinIx in order of first appearance over the ascending peptides; each peptide's sorted ProteinIx list
    std::unordered_map<uint32_t, uint32_t> protein_index;  // name * 2 + decoy -> ProteinIx
    std::vector<uint64_t> pep_off(n + 1, 0);
    std::vector<uint32_t> pep_list;
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t p = peptides[j];
        const uint8_t decoy = db.decoy[p] ? 1 : 0;
        const size_t lo = pep_list.size();
        for (uint64_t k = db.pep_protein_off[p]; k < db.pep_protein_off[p + 1]; ++k) {
            const uint32_t prot = db.pep_protein_ids[k];
            const uint32_t key = names.of_protein[prot] * 2u + decoy;
            auto it = protein_index.find(key);
            if (it == protein_index.end()) {
                it = protein_index.emplace(key, (uint32_t)out.protein_name.size()).first;
                out.protein_name.push_back(names.of_protein[prot]);
                out.protein_decoy.push_back(decoy);
                out.protein_db_id.push_back(prot);
            }
            pep_list.push_back(it->second);
        }
        std::sort(pep_list.begin() + lo, pep_list.end());
        pep_off[j + 1] = pep_list.size();
    }
    // the distinct lists in lexicographic order: a list's position is its meta-peptide index (:198)
    std::vector<uint32_t> by_list(n);
    std::iota(by_list.begin(), by_list.end(), 0u);
    const RowLess pep_less{pep_off, pep_list};
    std::sort(by_list.begin(), by_list.end(), pep_less);
    const uint32_t n_prot = (uint32_t)out.protein_name.size();
    // :197-202: every protein's evidence, the ascending meta-peptide indices it occurs in (once per occurrence)
    std::vector<uint64_t> ev_count(n_prot + 1, 0);
    std::vector<uint32_t> meta_rep;  // a peptide position that holds the meta-peptide's list
    for (uint64_t s = 0; s < n; ++s)
        if (s == 0 || pep_less.cmp(by_list[s - 1], by_list[s]) != 0) meta_rep.push_back(by_list[s]);
    out.n_meta = (uint32_t)meta_rep.size();
    for (uint32_t j : meta_rep)
        for (uint64_t k = pep_off[j]; k < pep_off[j + 1]; ++k) ev_count[pep_list[k] + 1]++;
    std::vector<uint64_t> ev_off(n_prot + 1, 0);
    for (uint32_t i = 0; i < n_prot; ++i) ev_off[i + 1] = ev_off[i] + ev_count[i + 1];
    std::vector<uint32_t> ev(ev_off[n_prot]);
    {
        std::vector<uint64_t> at(ev_off.begin(), ev_off.end() - 1);
        for (uint32_t m = 0; m < out.n_meta; ++m)
            for (uint64_t k = pep_off[meta_rep[m]]; k < pep_off[meta_rep[m] + 1]; ++k) ev[at[pep_list[k]]++] = m;
    }
    // :204-221: proteins with equal evidence are one group; the groups in the lexicographic order of their evidence
    std::vector<uint32_t> by_ev(n_prot);
    std::iota(by_ev.begin(), by_ev.end(), 0u);
    const RowLess ev_less{ev_off, ev};
    std::sort(by_ev.begin(), by_ev.end(), [&](uint32_t a, uint32_t b) {
        const int c = ev_less.cmp(a, b);
        return c != 0 ? c < 0 : a < b;
    });
    out.group_off.push_back(0);
    out.evidence_off.push_back(0);
    for (uint32_t s = 0; s < n_prot; ++s) {
        const uint32_t prot = by_ev[s];
        const bool first = s == 0 || ev_less.cmp(by_ev[s - 1], prot) != 0;
        if (first && s != 0) {
            out.group_off.push_back(out.group_proteins.size());
            out.evidence_off.push_back(out.evidence.size());
        }
        out.group_proteins.push_back(prot);
        if (first) {
            const uint32_t g = (uint32_t)(out.group_off.size() - 1);
            for (uint64_t k = ev_off[prot]; k < ev_off[prot + 1]; ++k) {
                out.evidence.push_back(ev[k]);
                out.edge_group.push_back(g);
                out.edge_meta.push_back(ev[k]);
            }
        }
    }
    if (n_prot) {
        out.group_off.push_back(out.group_proteins.size());
        out.evidence_off.push_back(out.evidence.size());
    } else {
        out.group_off.clear();  // no group at all: n_groups() == 0
        out.evidence_off.clear();
    }
}

std::string group_string(const HostDb& db, const GroupGraph& g, uint32_t group) {  // protein_grouping.rs:24-56
    std::vector<std::string> names;
    for (uint64_t k = g.group_off[group]; k < g.group_off[group + 1]; ++k) {
        const uint32_t ix = g.group_proteins[k];
        const std::string& name = db.protein_names[g.protein_db_id[ix]];
        names.push_back(g.protein_decoy[ix] && db.generate_decoys ? db.decoy_tag + name : name);
    }
    std::sort(names.begin(), names.end());
    std::string s;
    for (size_t i = 0; i < names.size(); ++i) {
        if (i) s += '/';
        s += names[i];
    }
    return s;
}

}  // namespace sagehip
