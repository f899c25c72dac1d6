// cover.h — the round logic of the greedy set cover of protein groups (left nodes) over meta-peptides (right nodes),
// crates/sage/src/protein_grouping.rs:59-156 (BipartiteGraph::into_cover), shared by the device kernels of protein_groups.hip and by the
// host (tests/hostemu/cover_emu.cpp runs it on the CPU).  Like core.h: plain functions, no HIP types.
//
//   into_cover   while edges remain: trim(); if edges remain: add_largest_to_cover()
//   trim         repeat until the number of edges stops changing:
//                  (a) every edge whose right node has degree 1 puts its left node into the cover          trim_force
//                  (b) every edge whose left node is covered is removed; its right node becomes covered    trim_left
//                  (c) every edge whose right node is covered is removed                                   trim_right
//   add_largest  the left node with the largest (remaining degree, original degree); Iterator::max_by_key returns the LAST
//                maximum, so a tie goes to the highest index: the largest CoverKey
//
// Inside one step no value that the step reads is written by it ((a) reads right degrees and writes the left cover, (b) reads
// the left cover and writes the right cover and the degrees, (c) reads the right cover and writes the degrees), so the edges of a
// step may be taken in any order, or all at once, as long as the steps themselves follow each other.  `A` says how memory is
// touched: plain on one host thread, device-scope atomics on the GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define COVER_HD __host__ __device__ __forceinline__
#else
#define COVER_HD inline
#endif

namespace sagecover {

struct Graph {             // node state; the edges are the caller's
    uint32_t* left_degree;   // [groups] current degree
    uint32_t* right_degree;  // [meta-peptides]
    uint32_t* left_cover;    // [groups] 0 / 1
    uint32_t* right_cover;   // [meta-peptides] 0 / 1
    const uint32_t* original_degree;  // [groups] the degree at construction (the tie-breaker)
};

struct PlainAccess {  // one thread
    static COVER_HD uint32_t load(const uint32_t* p) { return *p; }
    static COVER_HD void store(uint32_t* p, uint32_t v) { *p = v; }
    static COVER_HD void decrement(uint32_t* p) { *p -= 1u; }
};

template <class A>
COVER_HD void trim_force(const Graph& g, uint32_t l, uint32_t r) {  // (a)
    if (A::load(&g.right_degree[r]) == 1u) A::store(&g.left_cover[l], 1u);
}

template <class A>
COVER_HD bool trim_left(const Graph& g, uint32_t l, uint32_t r) {  // (b): true when the edge goes
    if (!A::load(&g.left_cover[l])) return false;
    A::store(&g.right_cover[r], 1u);
    A::decrement(&g.left_degree[l]);
    A::decrement(&g.right_degree[r]);
    return true;
}

template <class A>
COVER_HD bool trim_right(const Graph& g, uint32_t l, uint32_t r) {  // (c): true when the edge goes
    if (!A::load(&g.right_cover[r])) return false;
    A::decrement(&g.left_degree[l]);
    A::decrement(&g.right_degree[r]);
    return true;
}

struct CoverKey {  // ordered by (remaining, original, index); valid == 0 is below every key
    uint32_t remaining, original, index, valid;
};

COVER_HD CoverKey key_none() { return CoverKey{0u, 0u, 0u, 0u}; }

COVER_HD bool key_less(const CoverKey& a, const CoverKey& b) {
    if (a.valid != b.valid) return a.valid < b.valid;
    if (a.remaining != b.remaining) return a.remaining < b.remaining;
    if (a.original != b.original) return a.original < b.original;
    return a.index < b.index;
}

COVER_HD CoverKey key_max(const CoverKey& a, const CoverKey& b) { return key_less(a, b) ? b : a; }

template <class A>
COVER_HD CoverKey key_of(const Graph& g, uint32_t l) {
    return CoverKey{A::load(&g.left_degree[l]), g.original_degree[l], l, 1u};
}

}  // namespace sagecover
