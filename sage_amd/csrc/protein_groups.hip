// protein_groups.hip — sage_hip_protein_groups on the device.
// ======================================================================================================================
// Protein groups and picked protein-group FDR (sage-cli runner.rs:539-549; protein_grouping.rs:59-386, fdr.rs:192-226).
// Division of labour as in rescore.hip: the host (groups.cpp) orders vectors and builds strings, the device does what is per PSM
// or per edge — the selection of a pass, the set cover over the host-built edge list, the per-peptide lookup of covered groups,
// the gather of the competition keys and picked() (rescore.hip's, through post_search.h).  The round logic of the cover is
// cover.h's, shared with the host emulation.
// ======================================================================================================================
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <unordered_map>
#include <vector>

#include "cover.h"
#include "host_db.hpp"
#include "post_search.h"

namespace sagehip {

namespace {

constexpr uint32_t NONE32 = 0xFFFFFFFFu;
constexpr uint32_t COVER_LDS_DEFAULT = 16384;  // live edges at which one workgroup takes over: 128 KiB of the CU's 160 KiB of LDS
constexpr uint32_t COVER_LDS_MAX = 18432;      // 144 KiB; the rest is the kernel's bookkeeping and the runtime's
constexpr int CG_THREADS = 1024;               // the endgame workgroup
constexpr int CG_WAVES = CG_THREADS / 64;

struct DeviceAccess {  // device-scope relaxed atomics: every route sees the degrees and flags the others wrote, past any L1
    static __device__ __forceinline__ uint32_t load(const uint32_t* p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void store(uint32_t* p, uint32_t v) {
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void decrement(uint32_t* p) { atomicSub(p, 1u); }
};

// annotate_features' filter (protein_grouping.rs:349-353): flag[peptide] = 1 for label != -1 && peptide_q < threshold (a NaN
// compares false).  threshold < 0: every feature's peptide (the peptides that occur in the run).
__global__ __launch_bounds__(RB) void group_select_kernel(const SageFeature* __restrict__ f, const float* __restrict__ peptide_q, uint64_t n,
                                                          float threshold, uint32_t n_peptides, uint32_t* __restrict__ flag,
                                                          uint32_t* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = f[i].peptide_idx;
    if (p >= n_peptides) {
        atomicAdd(bad, 1u);
        return;
    }
    if (threshold < 0.0f || (f[i].label != -1 && peptide_q[i] < threshold)) flag[p] = 1u;
}

// the flagged peptides in ascending order: list[pos[p]] = p
__global__ __launch_bounds__(RB) void group_compact_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                           uint32_t n_peptides, uint32_t* __restrict__ list) {
    const uint32_t p = blockIdx.x * RB + threadIdx.x;
    if (p < n_peptides && flag[p]) list[pos[p]] = p;
}

// ---- the cover, bulk route: one kernel per trim step over the whole edge list with a live flag per edge --------------------
__global__ __launch_bounds__(RB) void cover_degrees_kernel(const uint32_t* __restrict__ el, const uint32_t* __restrict__ er, uint32_t n_edges,
                                                           uint32_t* __restrict__ left_degree, uint32_t* __restrict__ right_degree) {
    const uint32_t e = blockIdx.x * RB + threadIdx.x;
    if (e >= n_edges) return;
    atomicAdd(&left_degree[el[e]], 1u);
    atomicAdd(&right_degree[er[e]], 1u);
}

template <int STEP>  // 0: trim_force, 1: trim_left, 2: trim_right
__global__ __launch_bounds__(RB) void cover_trim_kernel(const uint32_t* __restrict__ el, const uint32_t* __restrict__ er, uint32_t n_edges,
                                                        uint8_t* __restrict__ live, sagecover::Graph g, uint32_t* __restrict__ n_live) {
    const uint32_t e = blockIdx.x * RB + threadIdx.x;
    bool gone = false;
    if (e < n_edges && live[e]) {
        const uint32_t l = el[e], r = er[e];
        if (STEP == 0) sagecover::trim_force<DeviceAccess>(g, l, r);
        else if (STEP == 1) gone = sagecover::trim_left<DeviceAccess>(g, l, r);
        else gone = sagecover::trim_right<DeviceAccess>(g, l, r);
        if (gone) live[e] = 0;
    }
    if (STEP != 0) {
        const unsigned long long b = __ballot(gone);
        if ((threadIdx.x & 63) == 0 && b) atomicSub(n_live, (uint32_t)__popcll(b));
    }
}

__device__ inline sagecover::CoverKey wave_key_max(sagecover::CoverKey k) {
    for (int o = 32; o > 0; o >>= 1) {
        sagecover::CoverKey other;
        other.remaining = __shfl_down(k.remaining, o, 64);
        other.original = __shfl_down(k.original, o, 64);
        other.index = __shfl_down(k.index, o, 64);
        other.valid = __shfl_down(k.valid, o, 64);
        k = sagecover::key_max(k, other);
    }
    return k;
}

// add_largest_to_cover, first half: partial[b] = the largest key of the block's left nodes
constexpr int COVER_PARTIALS = 256;
__global__ __launch_bounds__(RB) void cover_argmax_kernel(sagecover::Graph g, uint32_t n_groups, sagecover::CoverKey* __restrict__ partial) {
    __shared__ sagecover::CoverKey wk[RB / 64];
    sagecover::CoverKey k = sagecover::key_none();
    for (uint32_t l = blockIdx.x * RB + threadIdx.x; l < n_groups; l += gridDim.x * RB)
        k = sagecover::key_max(k, sagecover::key_of<DeviceAccess>(g, l));
    k = wave_key_max(k);
    if ((threadIdx.x & 63) == 0) wk[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RB / 64; ++w) k = sagecover::key_max(k, wk[w]);
        partial[blockIdx.x] = k;
    }
}
// second half: the largest partial enters the cover
__global__ __launch_bounds__(64) void cover_pick_kernel(sagecover::Graph g, const sagecover::CoverKey* __restrict__ partial, uint32_t n_partials) {
    sagecover::CoverKey k = sagecover::key_none();
    for (uint32_t b = threadIdx.x; b < n_partials; b += 64) k = sagecover::key_max(k, partial[b]);
    k = wave_key_max(k);
    if (threadIdx.x == 0 && k.valid) DeviceAccess::store(&g.left_cover[k.index], 1u);
}

// ---- the cover, endgame route: ONE workgroup runs every remaining round of into_cover with the live edges in LDS ------------
// The node state stays in global memory (a node index is not bounded by the cap), touched through DeviceAccess; the steps are
// separated by __syncthreads() only.  An edge that goes is overwritten with NONE32 in place.  Both loops are bounded: an outer round
// removes at least one edge, a trim repeat that removes none ends the trim.  out[0] += add_largest picks; out[1] = 0 done, 1 a bound was
// exceeded, 2 more live edges than `cap`.
__global__ __launch_bounds__(CG_THREADS) void cover_endgame_kernel(const uint32_t* __restrict__ el, const uint32_t* __restrict__ er,
                                                                   const uint8_t* __restrict__ live, uint32_t n_edges, uint32_t cap,
                                                                   sagecover::Graph g, uint32_t* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char cover_lds[];
    uint32_t* L = reinterpret_cast<uint32_t*>(cover_lds);
    uint32_t* R = L + cap;
    __shared__ uint32_t s_count;
    __shared__ uint32_t s_removed[2];
    __shared__ sagecover::CoverKey s_key[CG_WAVES];
    const uint32_t t = threadIdx.x;
    if (t == 0) s_count = 0;
    __syncthreads();
    for (uint32_t e = t; e < n_edges; e += CG_THREADS)
        if (live[e]) {
            const uint32_t slot = atomicAdd(&s_count, 1u);  // any order: every step is independent of the order of the edges
            if (slot < cap) {
                L[slot] = el[e];
                R[slot] = er[e];
            }
        }
    __syncthreads();
    const uint32_t n = s_count;
    if (n > cap) {
        if (t == 0) out[1] = 2;
        return;
    }
    uint32_t remaining = n, picks = 0, repeats = 0, status = 0;
    const uint32_t max_rounds = n + 1;
    for (uint32_t round = 0; remaining != 0; ++round) {
        if (round >= max_rounds) {
            status = 1;
            break;
        }
        for (;;) {  // trim()
            if (repeats > 2 * n + 2) {  // (every repeat but the last of a trim removes an edge)
                status = 1;
                break;
            }
            const uint32_t prev = remaining, par = repeats & 1u;
            ++repeats;
            if (t == 0) s_removed[par] = 0;
            for (uint32_t s = t; s < n; s += CG_THREADS)
                if (L[s] != NONE32) sagecover::trim_force<DeviceAccess>(g, L[s], R[s]);
            __syncthreads();
            uint32_t gone = 0;
            for (uint32_t s = t; s < n; s += CG_THREADS)
                if (L[s] != NONE32 && sagecover::trim_left<DeviceAccess>(g, L[s], R[s])) {
                    L[s] = NONE32;
                    ++gone;
                }
            __syncthreads();
            for (uint32_t s = t; s < n; s += CG_THREADS)
                if (L[s] != NONE32 && sagecover::trim_right<DeviceAccess>(g, L[s], R[s])) {
                    L[s] = NONE32;
                    ++gone;
                }
            if (gone) atomicAdd(&s_removed[par], gone);
            __syncthreads();
            remaining -= s_removed[par];  // (the other parity's counter is the one the next repeat resets)
            if (remaining == prev) break;
        }
        if (status || remaining == 0) break;
        sagecover::CoverKey k = sagecover::key_none();  // add_largest_to_cover: a left node with a live edge has remaining >= 1
        for (uint32_t s = t; s < n; s += CG_THREADS)
            if (L[s] != NONE32) k = sagecover::key_max(k, sagecover::key_of<DeviceAccess>(g, L[s]));
        k = wave_key_max(k);
        if ((t & 63) == 0) s_key[t >> 6] = k;
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < CG_WAVES; ++w) k = sagecover::key_max(k, s_key[w]);
            if (k.valid) DeviceAccess::store(&g.left_cover[k.index], 1u);
        }
        ++picks;
        __syncthreads();
    }
    if (t == 0) {
        out[0] += picks;
        out[1] = status;
    }
}

// ProteinGroupLookup::group_string's set (protein_grouping.rs:283-288) for peptide slot j of the run's peptides: hit[k] = the covered
// group of protein entry k of the slot, NONE32 without one; n_hit[j] = how many entries have one.  Assigned slots are skipped.
__global__ __launch_bounds__(RB) void group_lookup_kernel(const uint64_t* __restrict__ slot_off, const uint32_t* __restrict__ slot_key,
                                                          const uint8_t* __restrict__ assigned, uint32_t n_slots,
                                                          const uint32_t* __restrict__ key_group, const uint32_t* __restrict__ left_cover,
                                                          uint32_t* __restrict__ hit, uint32_t* __restrict__ n_hit) {
    const uint32_t j = blockIdx.x * RB + threadIdx.x;
    if (j >= n_slots) return;
    uint32_t c = 0;
    if (!assigned[j])
        for (uint64_t k = slot_off[j]; k < slot_off[j + 1]; ++k) {
            const uint32_t grp = key_group[slot_key[k]];
            const bool in = grp != NONE32 && left_cover[grp] != 0;
            hit[k] = in ? grp : NONE32;
            c += in;
        }
    n_hit[j] = c;
}

// first[slot] = the first feature (input order) of the slot's peptide; first is pre-filled with NONE32
__global__ __launch_bounds__(RB) void group_first_kernel(const SageFeature* __restrict__ f, uint64_t n, const uint32_t* __restrict__ slot_of,
                                                         uint32_t* __restrict__ first) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i < n) atomicMin(&first[slot_of[f[i].peptide_idx]], (uint32_t)i);
}

// per feature: the columns and the competition key / side of its peptide's slot
__global__ __launch_bounds__(RB) void group_gather_kernel(const SageFeature* __restrict__ f, uint64_t n, const uint32_t* __restrict__ slot_of,
                                                          const uint32_t* __restrict__ slot_key, const uint32_t* __restrict__ slot_num,
                                                          const uint32_t* __restrict__ slot_string, const uint8_t* __restrict__ slot_decoy,
                                                          uint32_t* __restrict__ key, uint8_t* __restrict__ decoy, uint32_t* __restrict__ num,
                                                          uint32_t* __restrict__ string_id) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot_of[f[i].peptide_idx];
    key[i] = slot_key[s];
    decoy[i] = slot_decoy[s];
    num[i] = slot_num[s];
    string_id[i] = slot_string[s];
}

uint32_t cover_lds_cap() {  // SAGE_HIP_COVER_LDS_EDGES, read once per call
    uint32_t cap = COVER_LDS_DEFAULT;
    if (const char* e = getenv("SAGE_HIP_COVER_LDS_EDGES")) {
        const long long v = atoll(e);
        cap = v <= 0 ? 0u : (uint32_t)std::min<long long>(v, COVER_LDS_MAX);
    }
    return cap;
}

// BipartiteGraph::new(edges, groups, meta-peptides).into_cover() on the device; d_left_cover [groups] receives the cover
bool cover_on_device(Ctx& cx, const GroupGraph& graph, uint32_t cap, uint32_t* d_left_cover, uint32_t& picks) {
    const uint32_t n_edges = (uint32_t)graph.edge_group.size(), n_groups = graph.n_groups(), n_meta = graph.n_meta;
    HIP_TRY(hipMemsetAsync(d_left_cover, 0, (size_t)std::max(n_groups, 1u) * 4, cx.stream));
    if (n_edges == 0) return true;
    Buf<uint32_t> el, er, ldeg, rdeg, odeg, rcov, counters;
    Buf<uint8_t> live;
    Buf<sagecover::CoverKey> partial;
    HIP_TRY(el.alloc(n_edges));
    HIP_TRY(er.alloc(n_edges));
    HIP_TRY(live.alloc(n_edges));
    HIP_TRY(ldeg.alloc(n_groups));
    HIP_TRY(odeg.alloc(n_groups));
    HIP_TRY(rdeg.alloc(n_meta));
    HIP_TRY(rcov.alloc(n_meta));
    HIP_TRY(counters.alloc(3));  // [0] add_largest picks of the endgame, [1] its status, [2] live edges
    HIP_TRY(partial.alloc(COVER_PARTIALS));
    HIP_TRY(hipMemcpyAsync(el.p, graph.edge_group.data(), (size_t)n_edges * 4, hipMemcpyHostToDevice, cx.stream));
    HIP_TRY(hipMemcpyAsync(er.p, graph.edge_meta.data(), (size_t)n_edges * 4, hipMemcpyHostToDevice, cx.stream));
    HIP_TRY(hipMemsetAsync(live.p, 1, n_edges, cx.stream));
    HIP_TRY(hipMemsetAsync(ldeg.p, 0, (size_t)n_groups * 4, cx.stream));
    HIP_TRY(hipMemsetAsync(rdeg.p, 0, (size_t)n_meta * 4, cx.stream));
    HIP_TRY(hipMemsetAsync(rcov.p, 0, (size_t)n_meta * 4, cx.stream));
    const uint32_t h_init[3] = {0, 0, n_edges};
    HIP_TRY(hipMemcpyAsync(counters.p, h_init, sizeof(h_init), hipMemcpyHostToDevice, cx.stream));
    const uint32_t ge = grid_for(n_edges, RB);
    cover_degrees_kernel<<<ge, RB, 0, cx.stream>>>(el.p, er.p, n_edges, ldeg.p, rdeg.p);
    HIP_TRY(hipMemcpyAsync(odeg.p, ldeg.p, (size_t)n_groups * 4, hipMemcpyDeviceToDevice, cx.stream));
    const sagecover::Graph g{ldeg.p, rdeg.p, d_left_cover, rcov.p, odeg.p};
    const uint32_t n_partials = std::min<uint32_t>(COVER_PARTIALS, grid_for(n_groups, RB));
    uint32_t live_edges = n_edges;
    auto read_live = [&]() -> bool {  // the one small counter the host loop reads per repeat
        HIP_TRY(hipMemcpyAsync(&live_edges, counters.p + 2, 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(cx.stream));
        return true;
    };
    picks = 0;
    for (uint64_t round = 0; live_edges != 0; ++round) {
        if (live_edges <= cap) {  // endgame: one workgroup, the live edges in LDS
            const size_t lds_bytes = (size_t)std::max(live_edges, 1u) * 8;
            if (lds_bytes > 64 * 1024)
                HIP_TRY(hipFuncSetAttribute((const void*)cover_endgame_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
            cover_endgame_kernel<<<1, CG_THREADS, lds_bytes, cx.stream>>>(el.p, er.p, live.p, n_edges, live_edges, g, counters.p);
            uint32_t h[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(h, counters.p, 8, hipMemcpyDeviceToHost, cx.stream));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(cx.stream));
            if (h[1] != 0) return cx.fail(SAGE_HIP_ERR_INTERNAL, "sage_hip_protein_groups: the set cover's endgame did not finish (status " +
                                                                     std::to_string(h[1]) + ")");
            picks += h[0];
            return true;
        }
        if (round > n_edges) return cx.fail(SAGE_HIP_ERR_INTERNAL, "sage_hip_protein_groups: the set cover did not finish in edges + 1 rounds");
        for (uint64_t repeat = 0;; ++repeat) {  // trim()
            if (repeat > n_edges) return cx.fail(SAGE_HIP_ERR_INTERNAL, "sage_hip_protein_groups: a trim did not finish in edges + 1 repeats");
            const uint32_t prev = live_edges;
            cover_trim_kernel<0><<<ge, RB, 0, cx.stream>>>(el.p, er.p, n_edges, live.p, g, counters.p + 2);
            cover_trim_kernel<1><<<ge, RB, 0, cx.stream>>>(el.p, er.p, n_edges, live.p, g, counters.p + 2);
            cover_trim_kernel<2><<<ge, RB, 0, cx.stream>>>(el.p, er.p, n_edges, live.p, g, counters.p + 2);
            if (!read_live()) return false;
            if (live_edges == prev || live_edges <= cap) break;  // (the endgame's first trim repeat is this trim's next one)
        }
        if (live_edges == 0 || live_edges <= cap) continue;
        cover_argmax_kernel<<<n_partials, RB, 0, cx.stream>>>(g, n_groups, partial.p);
        cover_pick_kernel<<<1, 64, 0, cx.stream>>>(g, partial.p, n_partials);
        ++picks;
    }
    return true;
}

struct GroupStringTable {  // the distinct protein_groups strings of a call, in order of first use
    std::vector<std::string> strings;
    std::unordered_map<std::string, uint32_t> ids;
    uint32_t intern(const std::string& s) {
        auto it = ids.find(s);
        if (it != ids.end()) return it->second;
        strings.push_back(s);
        return ids.emplace(s, (uint32_t)(strings.size() - 1)).first->second;
    }
};

bool protein_groups_impl(Ctx& cx, const HostDb& db, const SageGroupInput& in, SageGroupOutput& out, std::vector<std::string>& strings_out) {
    const uint64_t n = in.n;
    const uint32_t np = (uint32_t)db.n_peptides();
    const uint32_t cap = cover_lds_cap();
    Events<2> ev;
    HIP_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev[0], cx.stream));
    Buf<SageFeature> feats;
    Buf<float> pq, score;
    Buf<uint32_t> flag, pos, list, counters;
    HIP_TRY(feats.alloc(n));
    HIP_TRY(pq.alloc(n));
    HIP_TRY(score.alloc(n));
    HIP_TRY(flag.alloc(np));
    HIP_TRY(pos.alloc((size_t)np + 1));
    HIP_TRY(list.alloc(np));
    HIP_TRY(counters.alloc(1));
    HIP_TRY(hipMemcpyAsync(feats.p, in.features, n * sizeof(SageFeature), hipMemcpyHostToDevice, cx.stream));
    HIP_TRY(hipMemcpyAsync(pq.p, in.peptide_q, n * 4, hipMemcpyHostToDevice, cx.stream));
    HIP_TRY(hipMemcpyAsync(score.p, in.discriminant_score, n * 4, hipMemcpyHostToDevice, cx.stream));
    HIP_TRY(hipMemsetAsync(counters.p, 0, 4, cx.stream));
    const uint32_t gf = grid_for(n, RB), gp = grid_for(np, RB);

    // the flagged peptides, ascending: selection kernel, exclusive scan of the flags, compaction
    auto select = [&](float threshold, std::vector<uint32_t>& h_list) -> bool {
        HIP_TRY(hipMemsetAsync(flag.p, 0, (size_t)std::max(np, 1u) * 4, cx.stream));
        group_select_kernel<<<gf, RB, 0, cx.stream>>>(feats.p, pq.p, n, threshold, np, flag.p, counters.p);
        uint32_t h_bad = 0, last_pos = 0, last_flag = 0;
        if (np) {
            if (!exclusive_count(cx, flag.p, pos.p, np)) return false;
            group_compact_kernel<<<gp, RB, 0, cx.stream>>>(flag.p, pos.p, np, list.p);
            HIP_TRY(hipMemcpyAsync(&last_pos, pos.p + (np - 1), 4, hipMemcpyDeviceToHost, cx.stream));
            HIP_TRY(hipMemcpyAsync(&last_flag, flag.p + (np - 1), 4, hipMemcpyDeviceToHost, cx.stream));
        }
        HIP_TRY(hipMemcpyAsync(&h_bad, counters.p, 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(cx.stream));
        if (h_bad) return cx.fail(SAGE_HIP_ERR_INVALID, "sage_hip_protein_groups: a feature's peptide index is out of range");
        h_list.resize((size_t)last_pos + last_flag);
        if (!h_list.empty()) {
            HIP_TRY(hipMemcpyAsync(h_list.data(), list.p, h_list.size() * 4, hipMemcpyDeviceToHost, cx.stream));
            HIP_TRY(hipStreamSynchronize(cx.stream));
        }
        return true;
    };

    // the peptides that occur in the run: slot j = position in the ascending list; slot_of[peptide] = j
    std::vector<uint32_t> occ;
    if (!select(-1.0f, occ)) return false;
    const uint32_t n_slots = (uint32_t)occ.size();
    Buf<uint32_t> slot_of;
    HIP_TRY(slot_of.alloc((size_t)np + 1));
    HIP_TRY(hipMemcpyAsync(slot_of.p, pos.p, (size_t)np * 4, hipMemcpyDeviceToDevice, cx.stream));
    const NameIndex names(db);
    std::vector<uint64_t> slot_off(n_slots + 1, 0);
    std::vector<uint32_t> slot_key;  // per protein entry of a slot: name * 2 + decoy
    for (uint32_t j = 0; j < n_slots; ++j) {
        const uint64_t p = occ[j];
        for (uint64_t k = db.pep_protein_off[p]; k < db.pep_protein_off[p + 1]; ++k)
            slot_key.push_back(names.of_protein[db.pep_protein_ids[k]] * 2u + (db.decoy[p] ? 1u : 0u));
        slot_off[j + 1] = slot_key.size();
    }
    const uint64_t n_entries = slot_key.size();
    std::vector<uint8_t> assigned(n_slots, 0);
    std::vector<uint32_t> slot_string(n_slots, NONE32), slot_num(n_slots, 0);
    GroupStringTable table;
    out.n_groups = out.n_meta_peptides = out.cover_rounds = 0;
    out.host_graph_ms = 0.0;

    if (in.protein_grouping && n_slots) {
        Buf<uint64_t> d_slot_off;
        Buf<uint32_t> d_slot_key, d_key_group, d_cover, d_hit, d_nhit;
        Buf<uint8_t> d_assigned;
        HIP_TRY(d_slot_off.alloc((size_t)n_slots + 1));
        HIP_TRY(d_slot_key.alloc(n_entries));
        HIP_TRY(d_key_group.alloc((size_t)names.n_names * 2));
        HIP_TRY(d_hit.alloc(n_entries));
        HIP_TRY(d_nhit.alloc(n_slots));
        HIP_TRY(d_assigned.alloc(n_slots));
        HIP_TRY(hipMemcpyAsync(d_slot_off.p, slot_off.data(), ((size_t)n_slots + 1) * 8, hipMemcpyHostToDevice, cx.stream));
        if (n_entries) HIP_TRY(hipMemcpyAsync(d_slot_key.p, slot_key.data(), n_entries * 4, hipMemcpyHostToDevice, cx.stream));
        float t1 = in.peptide_fdr;  // f32::clamp(0.0, 1.0): a NaN stays a NaN and selects nothing
        if (t1 < 0.0f) t1 = 0.0f;
        if (t1 > 1.0f) t1 = 1.0f;
        const float thresholds[2] = {t1, 1.0f};
        std::vector<uint32_t> selected, key_group((size_t)names.n_names * 2), h_hit(n_entries), h_nhit(n_slots);
        for (int pass = 0; pass < 2; ++pass) {
            if (thresholds[pass] != thresholds[pass]) selected.clear();
            else if (!select(thresholds[pass], selected)) return false;
            const auto t0 = std::chrono::steady_clock::now();
            GroupGraph graph;
            build_group_graph(db, names, selected.data(), selected.size(), graph);
            std::fill(key_group.begin(), key_group.end(), NONE32);
            const uint32_t n_groups = graph.n_groups();
            for (uint32_t grp = 0; grp < n_groups; ++grp)
                for (uint64_t k = graph.group_off[grp]; k < graph.group_off[grp + 1]; ++k) {
                    const uint32_t ix = graph.group_proteins[k];
                    key_group[graph.protein_name[ix] * 2u + graph.protein_decoy[ix]] = grp;
                }
            out.host_graph_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            out.n_groups = n_groups;
            out.n_meta_peptides = graph.n_meta;
            if (n_groups == 0) continue;  // nothing selected: nothing can be annotated
            HIP_TRY(d_cover.alloc(n_groups));
            uint32_t picks = 0;
            if (!cover_on_device(cx, graph, cap, d_cover.p, picks)) return false;
            out.cover_rounds += picks;
            HIP_TRY(hipMemcpyAsync(d_key_group.p, key_group.data(), key_group.size() * 4, hipMemcpyHostToDevice, cx.stream));
            HIP_TRY(hipMemcpyAsync(d_assigned.p, assigned.data(), n_slots, hipMemcpyHostToDevice, cx.stream));
            group_lookup_kernel<<<grid_for(n_slots, RB), RB, 0, cx.stream>>>(d_slot_off.p, d_slot_key.p, d_assigned.p, n_slots, d_key_group.p,
                                                                            d_cover.p, d_hit.p, d_nhit.p);
            if (n_entries) HIP_TRY(hipMemcpyAsync(h_hit.data(), d_hit.p, n_entries * 4, hipMemcpyDeviceToHost, cx.stream));
            HIP_TRY(hipMemcpyAsync(h_nhit.data(), d_nhit.p, (size_t)n_slots * 4, hipMemcpyDeviceToHost, cx.stream));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(cx.stream));
            // the strings, once per distinct peptide (protein_grouping.rs:290-300, :372-373)
            std::vector<std::string> group_str(n_groups);
            std::vector<uint8_t> have(n_groups, 0);
            std::vector<uint32_t> set;
            std::vector<std::string> parts;
            for (uint32_t j = 0; j < n_slots; ++j) {
                if (assigned[j] || h_nhit[j] == 0) continue;
                set.clear();
                for (uint64_t k = slot_off[j]; k < slot_off[j + 1]; ++k)
                    if (h_hit[k] != NONE32) set.push_back(h_hit[k]);
                std::sort(set.begin(), set.end());
                set.erase(std::unique(set.begin(), set.end()), set.end());
                parts.clear();
                for (uint32_t grp : set) {
                    if (!have[grp]) {
                        group_str[grp] = group_string(db, graph, grp);
                        have[grp] = 1;
                    }
                    parts.push_back(group_str[grp]);
                }
                std::sort(parts.begin(), parts.end());
                std::string s;
                for (size_t i = 0; i < parts.size(); ++i) {
                    if (i) s += ';';
                    s += parts[i];
                }
                slot_num[j] = (uint32_t)std::count(s.begin(), s.end(), ';') + 1u;
                slot_string[j] = table.intern(s);
                assigned[j] = 1;
            }
        }
    }
    // the fallback (protein_grouping.rs:326-334)
    for (uint32_t j = 0; j < n_slots; ++j)
        if (!assigned[j]) {
            slot_string[j] = table.intern(db.peptide_proteins(occ[j]));
            slot_num[j] = (uint32_t)(db.pep_protein_off[occ[j] + 1] - db.pep_protein_off[occ[j]]);
        }
    // picked_protein_group: dense keys by string equality over the slots whose count is 1, numbered in the order in which the
    // features first use them (the numbering of HostDb::competition_keys; it fixes the order of the KDE's sums)
    std::vector<uint32_t> slot_first(n_slots, NONE32);
    {
        Buf<uint32_t> d_first;
        HIP_TRY(d_first.alloc(n_slots));
        HIP_TRY(hipMemsetAsync(d_first.p, 0xFF, (size_t)std::max(n_slots, 1u) * 4, cx.stream));
        group_first_kernel<<<gf, RB, 0, cx.stream>>>(feats.p, n, slot_of.p, d_first.p);
        if (n_slots) HIP_TRY(hipMemcpyAsync(slot_first.data(), d_first.p, (size_t)n_slots * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(cx.stream));
    }
    std::vector<uint32_t> comp_key(n_slots, NONE32), key_of_string(table.strings.size(), NONE32), first_of_string(table.strings.size(), NONE32);
    std::vector<uint8_t> slot_decoy(n_slots, 0);
    std::vector<uint32_t> competing;  // string ids
    for (uint32_t j = 0; j < n_slots; ++j) {
        slot_decoy[j] = db.decoy[occ[j]] ? 1 : 0;
        if (slot_num[j] != 1) continue;
        uint32_t& first = first_of_string[slot_string[j]];
        if (first == NONE32) competing.push_back(slot_string[j]);
        first = std::min(first, slot_first[j]);  // (every slot has a feature, so the minimum is one)
    }
    std::sort(competing.begin(), competing.end(), [&](uint32_t a, uint32_t b) { return first_of_string[a] < first_of_string[b]; });
    const uint32_t n_keys = (uint32_t)competing.size();
    for (uint32_t k = 0; k < n_keys; ++k) key_of_string[competing[k]] = k;
    for (uint32_t j = 0; j < n_slots; ++j)
        if (slot_num[j] == 1) comp_key[j] = key_of_string[slot_string[j]];
    Buf<uint32_t> d_comp_key, d_slot_num, d_slot_string, d_key, d_num, d_string;
    Buf<uint8_t> d_slot_decoy, d_decoy;
    Buf<float> d_q;
    HIP_TRY(d_comp_key.alloc(n_slots));
    HIP_TRY(d_slot_num.alloc(n_slots));
    HIP_TRY(d_slot_string.alloc(n_slots));
    HIP_TRY(d_slot_decoy.alloc(n_slots));
    HIP_TRY(d_key.alloc(n));
    HIP_TRY(d_num.alloc(n));
    HIP_TRY(d_string.alloc(n));
    HIP_TRY(d_decoy.alloc(n));
    HIP_TRY(d_q.alloc(n));
    if (n_slots) {
        HIP_TRY(hipMemcpyAsync(d_comp_key.p, comp_key.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_slot_num.p, slot_num.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_slot_string.p, slot_string.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_slot_decoy.p, slot_decoy.data(), n_slots, hipMemcpyHostToDevice, cx.stream));
    }
    group_gather_kernel<<<gf, RB, 0, cx.stream>>>(feats.p, n, slot_of.p, d_comp_key.p, d_slot_num.p, d_slot_string.p, d_slot_decoy.p, d_key.p,
                                                  d_decoy.p, d_num.p, d_string.p);
    uint64_t passing = 0;
    if (!picked(cx, d_key.p, n_keys, d_decoy.p, score.p, n, d_q.p, passing)) return false;
    out.passing_protein_group = passing;
    HIP_TRY(hipMemcpyAsync(out.num_protein_groups, d_num.p, n * 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(out.string_id, d_string.p, n * 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(out.protein_group_q, d_q.p, n * 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipEventRecord(ev[1], cx.stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(cx.stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    out.device_ms = ms;
    strings_out = std::move(table.strings);
    return true;
}

}  // namespace

// entry point used by capi_host.cpp; returns a SAGE_HIP_* status, message in `err`
int protein_groups_on_device(int device, const HostDb& db, const SageGroupInput& in, SageGroupOutput& out, std::vector<std::string>& strings,
                             std::string& err) {
    return run_on_device<ScratchScope>(device, "sage_hip_protein_groups", "sage_hip_protein_groups: ", err,
                                       [&](Ctx& cx) { return protein_groups_impl(cx, db, in, out, strings); });
}

}  // namespace sagehip
