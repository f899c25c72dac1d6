// What the post-search translation units share: rescore.hip (PSM rescoring), rt_model.hip (sage_hip_predict_rt) and
// protein_groups.hip (sage_hip_protein_groups).  Host and device code: the launch geometry, the block reduction, the pooled
// scratch buffer of a call, and the host helpers that rescore.hip defines and the other two call (the rocPRIM scans and the
// 32-bit sort are instantiated there only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "hip_host.h"

namespace sagehip {

constexpr int RB = 256;          // threads of a row-parallel block
constexpr int MAX_BLOCKS = 512;  // partials per (order-free) reduction

inline uint32_t grid_for(uint64_t n, uint32_t block) { return (uint32_t)std::max<uint64_t>(1, (n + block - 1) / block); }
inline uint32_t blocks_for(uint64_t n) { return (uint32_t)std::min<uint64_t>(MAX_BLOCKS, std::max<uint64_t>(1, (n + RB - 1) / RB)); }

struct OpSum {
    __device__ double operator()(double a, double b) const { return a + b; }
};
struct OpMin {
    __device__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct OpMax {
    __device__ double operator()(double a, double b) const { return fmax(a, b); }
};

// fixed-tree block reduction (wave shuffles, then the wave results through LDS); result valid in thread 0
template <class Op>
__device__ inline double block_reduce(double v, Op op, double* lds /* >= blockDim/64 doubles */) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o, 64));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < nw; ++w) v = op(v, lds[w]);
    return v;
}

// Device scratch of one call.  Allocations are stream-ordered (hipMallocAsync / hipFreeAsync on the call's stream) out of
// the device's default memory pool, whose release threshold is raised once so that freed blocks stay cached between
// calls: after the first call a rescoring allocates nothing from the driver (the ~30 hipMalloc / hipFree pairs used to be a
// third of the wall time of a 1 M-PSM call).  SAGE_HIP_NO_POOL=1 falls back to plain hipMalloc / hipFree.
//
// ScratchScope (rescore.hip) names the pool and the stream of the call that runs on this thread, from the call's entry until it
// returns; SAGE_HIP_NO_POOL is read there, once per call.  Outside a scope every allocation is a plain hipMalloc.
struct ScratchScope {
    ScratchScope(int device, hipStream_t stream);
    ~ScratchScope();
    ScratchScope(const ScratchScope&) = delete;
    ScratchScope& operator=(const ScratchScope&) = delete;
};
// `bytes` of scratch for the call in scope: *pool_stream = the stream the block is ordered on (free it with hipFreeAsync there), or
// null for a block of hipMalloc's, which is also what a failed hipMallocAsync falls back to
hipError_t scratch_alloc(void** p, size_t bytes, hipStream_t* pool_stream);

template <class T>
struct Buf {
    T* p = nullptr;
    hipStream_t pool_stream = nullptr;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    void release() {
        if (!p) return;
        if (pool_stream) (void)hipFreeAsync(p, pool_stream);  // ordered after every kernel of this call that uses it
        else (void)hipFree(p);
        p = nullptr;
    }
    hipError_t alloc(size_t count) {
        release();
        return scratch_alloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T), &pool_stream);
    }
};

// Gauss::solve (gauss.rs:27-165): the identical elimination order and epsilon ladder, because the solution of the regularised
// system depends on both
struct Dense {
    std::vector<double> a;
    size_t rows, cols;
    Dense(size_t r, size_t c) : a(r * c, 0.0), rows(r), cols(c) {}
    double& at(size_t i, size_t j) { return a[i * cols + j]; }
    void swap_rows(size_t i, size_t j) {
        for (size_t k = 0; k < cols; ++k) std::swap(at(i, k), at(j, k));
    }
};
bool gauss_solve(const Dense& left, const Dense& right, std::vector<double>& out);

// out[j] = sum of flags[0..j]; synchronises the stream
bool prefix_count(Ctx& cx, const uint32_t* d_flags, uint32_t* d_out, uint32_t n);
// out[j] = sum of flags[0..j)
bool exclusive_count(Ctx& cx, const uint32_t* d_flags, uint32_t* d_out, uint64_t n);
// spectrum_q_value (ml/qvalue.rs:8-36) of `n` PSMs whose d_order[j] is the index of the j-th best: d_q_out[i] in input order.
// d_flags / d_cum and d_q_sorted / d_qmin_sorted are scratch of n elements each; d_qmin_sorted keeps the q-values in sorted order.
// With d_passing, *d_passing = the number of PSMs at q <= 0.01, counted before the scatter.
bool spectrum_q_values(Ctx& cx, const uint32_t* d_order, const uint8_t* d_decoy, uint32_t n, uint32_t* d_flags, uint32_t* d_cum,
                       float* d_q_sorted, float* d_qmin_sorted, float* d_q_out, unsigned long long* d_passing = nullptr);
// Competition::assign_q_value over dense keys (fdr.rs:60-120) and the write-back of fdr.rs:146-148 / :179-185
bool picked(Ctx& cx, const uint32_t* d_key, uint32_t n_keys, const uint8_t* d_decoy, const float* d_score, uint64_t n, float* d_q_out,
            uint64_t& passing);

}  // namespace sagehip
