// protein_lfq.hip — the protein-level roll-up of label-free quantification on the device (MaxLFQ): per protein
// and pair of files the median of the log-ratios over the shared precursor rows, then per protein the least-squares abundances
// of its files, anchored to the observed log intensities.  The arithmetic is maxlfq.h's, which the host emulation shares.
//
//   plfq_log_kernel          L[file][grouped row] = cr_log(area) or NaN (missing), once per cell; the rows are grouped by protein
//                            with a stable radix sort (rocPRIM), so a protein's rows are one range of every file's column and a
//                            pair of files is two contiguous streams.
//   plfq_pair_median_kernel  one wavefront per (protein, pair of files).  One pass over the two columns forms the differences of
//                            the shared rows as order-preserving u64 keys (maxlfq::key_of), compacted by ballot into the wave's
//                            LDS slice while the protein has at most PLFQ_LDS_KEYS rows.  The median's two ranks are selected
//                            exactly and wave-uniformly: up to 64 keys, one per lane, by counting with ballots; beyond that by
//                            a bitwise radix select (maxlfq::radix_select) over the LDS slice, or — a protein of more rows — over
//                            the two columns read again (those proteins in a launch of their own, one pair per wavefront).  No
//                            floating-point atomics, nothing that depends on arrival order.
//   plfq_solve_kernel        one workgroup per protein: maxlfq::column_sums and maxlfq::solve with the workgroup as the Team.
//                            The augmented matrix and the factor vector live in LDS while they fit PLFQ_LDS_BYTES, else in a
//                            slot of a global workspace; the code is the same.
//
// Proteins are processed in batches whose pair tables, results and workspace stay below SAGE_HIP_PLFQ_WORKSPACE_MB.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <rocprim/device/device_radix_sort.hpp>

#include "device_types.h"
#include "hip_host.h"
#include "maxlfq.h"

namespace sagehip {

namespace {

constexpr uint32_t PLFQ_THREADS = 256;
constexpr uint32_t PLFQ_WAVES = PLFQ_THREADS / 64;
constexpr uint32_t PLFQ_LDS_KEYS = 1024;        // keys a wavefront stages in LDS (8 KB per wave, 32 KB per workgroup)
constexpr uint32_t PLFQ_PAIRS_PER_WAVE = 16;    // consecutive pairs one wavefront works through
constexpr uint32_t PLFQ_PAIRS_PER_BLOCK = PLFQ_WAVES * PLFQ_PAIRS_PER_WAVE;
constexpr uint32_t PLFQ_LDS_BYTES = 64 * 1024;  // of the solve kernel's matrix + factors: n (n + 2) * 8 bytes, n <= 89
constexpr uint32_t PLFQ_MAX_SLOTS = 1024;       // workgroups of the solve kernel in flight
constexpr double PLFQ_DEFAULT_MB = 512.0;

__global__ __launch_bounds__(PLFQ_THREADS) void plfq_iota_kernel(uint32_t n, uint32_t* out) {
    const uint32_t i = blockIdx.x * PLFQ_THREADS + threadIdx.x;
    if (i < n) out[i] = i;
}

// L[f * n_used + g] for the g-th row in grouped order (row[g] of the input), g < n_used
__global__ __launch_bounds__(PLFQ_THREADS) void plfq_log_kernel(uint32_t n_used, uint32_t n_files, const double* __restrict__ areas,
                                                                 const uint32_t* __restrict__ row, double* __restrict__ L) {
    const uint64_t cell = (uint64_t)blockIdx.x * PLFQ_THREADS + threadIdx.x;
    if (cell >= (uint64_t)n_used * n_files) return;
    const uint32_t f = (uint32_t)(cell / n_used), g = (uint32_t)(cell % n_used);
    L[cell] = maxlfq::log_of_area(areas[(uint64_t)row[g] * n_files + f]);
}

// LDS writes of some lanes of a wavefront, read by others of the same wavefront afterwards
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// Proteins first .. first + n_prot of the batch; off: the row range of every protein in grouped order; med / cnt: [n_prot * P].
// Two launches: without long_list every protein of the batch, pairs_per_wave consecutive pairs per wavefront, where a protein of
// more than PLFQ_LDS_KEYS rows is passed over; with long_list (the batch's indices of exactly those proteins) one pair per
// wavefront, since each of their pairs costs up to 128 passes over two columns.
__global__ __launch_bounds__(PLFQ_THREADS) void plfq_pair_median_kernel(const double* __restrict__ L, uint64_t stride,
                                                                         const uint64_t* __restrict__ off, uint32_t first, uint32_t n,
                                                                         uint32_t slices, uint32_t min_count, double* __restrict__ med,
                                                                         uint32_t* __restrict__ cnt, const uint32_t* __restrict__ long_list,
                                                                         uint32_t pairs_per_wave) {
    __shared__ uint64_t lds_keys[PLFQ_WAVES][PLFQ_LDS_KEYS];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t lp = long_list ? long_list[blockIdx.x / slices] : blockIdx.x / slices, slice = blockIdx.x % slices;
    const uint64_t P = maxlfq::n_pairs(n);
    uint64_t q = ((uint64_t)slice * PLFQ_WAVES + w) * pairs_per_wave;
    if (q >= P) return;  // (wave-uniform: there is no workgroup barrier below)
    const uint64_t a = off[first + lp];
    const uint32_t nr = (uint32_t)(off[first + lp + 1] - a);
    const bool staged = nr <= PLFQ_LDS_KEYS;
    if (staged != (long_list == nullptr)) return;  // a long protein's pairs belong to the launch over long_list, one per wavefront
    uint64_t* keys = lds_keys[w];
    // (j, k) of pair q, then one step per pair
    uint32_t j = 0;
    {
        uint64_t left = q;
        while (left >= n - 1 - j) {
            left -= n - 1 - j;
            ++j;
        }
        uint32_t k = j + 1 + (uint32_t)left;
        for (uint32_t step = 0; step < pairs_per_wave && q < P; ++step, ++q) {
            const double* Lj = L + (uint64_t)j * stride + a;
            const double* Lk = L + (uint64_t)k * stride + a;
            uint32_t c = 0;
            for (uint32_t base = 0; base < nr; base += 64) {
                const uint32_t r = base + lane;
                double x = maxlfq::missing(), y = x;
                if (r < nr) {
                    x = Lj[r];
                    y = Lk[r];
                }
                const bool both = maxlfq::present(x) && maxlfq::present(y);
                const uint64_t mask = __ballot(both);
                if (staged && both) keys[c + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = maxlfq::key_of(x - y);
                c += (uint32_t)__popcll(mask);
            }
            wave_sync();
            double m = maxlfq::missing();
            if (c >= min_count) {  // (wave-uniform)
                const uint32_t rank_lo = (c - 1) / 2, rank_hi = c / 2;
                uint64_t klo = 0, khi = 0;
                if (staged && c <= 64) {
                    // one key per lane; for every key v, how many keys lie below it and how many do not lie above it
                    const bool own = lane < c;
                    const uint64_t mine = own ? keys[lane] : 0;
                    for (uint32_t i = 0; i < c; ++i) {
                        const uint64_t v = keys[i];
                        const uint32_t below = wave_count(own && mine < v), upto = wave_count(own && mine <= v);
                        if (below <= rank_lo && rank_lo < upto) klo = v;
                        if (below <= rank_hi && rank_hi < upto) khi = v;
                    }
                } else if (staged) {
                    auto zeros = [&](uint64_t prefix, int bit) {
                        uint32_t z = 0;
                        for (uint32_t base = 0; base < c; base += 64) {
                            const uint32_t i = base + lane;
                            z += wave_count(i < c && (keys[i < c ? i : 0] >> bit) == (prefix >> bit));
                        }
                        return z;
                    };
                    klo = maxlfq::radix_select(rank_lo, zeros);
                    khi = rank_hi == rank_lo ? klo : maxlfq::radix_select(rank_hi, zeros);
                } else {
                    auto zeros = [&](uint64_t prefix, int bit) {
                        uint32_t z = 0;
                        for (uint32_t base = 0; base < nr; base += 64) {
                            const uint32_t r = base + lane;
                            double x = maxlfq::missing(), y = x;
                            if (r < nr) {
                                x = Lj[r];
                                y = Lk[r];
                            }
                            const bool both = maxlfq::present(x) && maxlfq::present(y);
                            z += wave_count(both && (maxlfq::key_of(x - y) >> bit) == (prefix >> bit));
                        }
                        return z;
                    };
                    klo = maxlfq::radix_select(rank_lo, zeros);
                    khi = rank_hi == rank_lo ? klo : maxlfq::radix_select(rank_hi, zeros);
                }
                m = maxlfq::median_of(maxlfq::of_key(klo), maxlfq::of_key(khi), c);
            }
            if (lane == 0) {
                med[(uint64_t)lp * P + q] = m;
                cnt[(uint64_t)lp * P + q] = c;
            }
            wave_sync();  // (the next pair writes the keys again)
            if (++k == n) {
                ++j;
                k = j + 1;
            }
        }
    }
}

struct WorkgroupTeam {
    __device__ uint32_t rank() const { return threadIdx.x; }
    __device__ uint32_t size() const { return blockDim.x; }
    __device__ void sync() const { __syncthreads(); }
    __device__ bool any(bool mine) const { return __syncthreads_or(mine ? 1 : 0) != 0; }
};

// One workgroup per protein of the batch (grid-stride: a workgroup owns slot blockIdx.x of the workspace).  in_lds: matrix and
// factors in dynamic LDS; else ws[slot * (n (n + 2))].  bad_pivot: 0, or 1 + the largest protein whose elimination met a zero or
// non-finite pivot (an integer maximum: the same value in any order).
__global__ __launch_bounds__(PLFQ_THREADS) void plfq_solve_kernel(const double* __restrict__ L, uint64_t stride,
                                                                   const uint64_t* __restrict__ off, uint32_t first, uint32_t n_prot,
                                                                   uint32_t n, uint32_t min_count, const double* __restrict__ med,
                                                                   const uint32_t* __restrict__ cnt, int in_lds, double* __restrict__ ws,
                                                                   double* __restrict__ col, uint32_t* __restrict__ ncol,
                                                                   double* __restrict__ log_abundance, double* __restrict__ intensity,
                                                                   uint32_t* __restrict__ component, uint32_t* __restrict__ n_rows_used,
                                                                   uint32_t* __restrict__ n_components, uint32_t* __restrict__ bad_pivot) {
    extern __shared__ double plfq_lds[];
    const WorkgroupTeam team;
    const uint64_t P = maxlfq::n_pairs(n), cells = (uint64_t)n * (n + 1);
    double* A = in_lds ? plfq_lds : ws + (uint64_t)blockIdx.x * (cells + n);
    for (uint32_t lp = blockIdx.x; lp < n_prot; lp += gridDim.x) {
        const uint64_t a = off[first + lp];
        const uint32_t nr = (uint32_t)(off[first + lp + 1] - a);
        const uint64_t o = (uint64_t)lp * n;
        maxlfq::column_sums(team, L + a, stride, nr, n, col + o, ncol + o);
        team.sync();
        const maxlfq::Protein v{n, min_count, med + (uint64_t)lp * P, cnt + (uint64_t)lp * P, col + o, ncol + o, A, A + cells,
                                log_abundance + o, intensity + o, component + o};
        const uint32_t bad = maxlfq::solve(team, v, n_components + lp);
        if (threadIdx.x == 0) {
            n_rows_used[lp] = nr;
            if (bad) atomicMax(bad_pivot, first + lp + 1);
        }
        team.sync();
    }
}

double workspace_budget_bytes() {
    double mb = PLFQ_DEFAULT_MB;
    if (const char* s = std::getenv("SAGE_HIP_PLFQ_WORKSPACE_MB")) {
        char* end = nullptr;
        const double v = std::strtod(s, &end);
        if (end != s && v > 0.0 && std::isfinite(v)) mb = v;
    }
    return mb * 1024.0 * 1024.0;
}

bool protein_lfq_impl(Ctx& cx, int device, const SageProteinLfqInput& in, SageProteinLfqOutput& out) {
    const uint32_t n = in.n_files, NP = in.n_proteins;
    const uint64_t P = maxlfq::n_pairs(n);
    const uint32_t mc = in.min_ratio_count ? in.min_ratio_count : 1;
    // rows per protein: the offsets of the grouped order (and the one check that needs every id)
    std::vector<uint64_t> off((size_t)NP + 1, 0);
    for (uint64_t r = 0; r < in.n_rows; ++r) {
        const uint32_t p = in.protein_of_row[r];
        if (p == maxlfq::NONE) continue;
        if (p >= NP) return cx.fail(SAGE_HIP_ERR_INVALID, "sage_hip_protein_lfq: protein id " + std::to_string(p) + " of row " +
                                                              std::to_string(r) + " is not below n_proteins");
        ++off[(size_t)p + 1];
    }
    for (uint32_t p = 0; p < NP; ++p) off[(size_t)p + 1] += off[p];
    const uint64_t n_used = off[NP];
    const uint32_t n_rows = (uint32_t)in.n_rows;  // (< 2^31: the entry point's guard)

    HIP_TRY(hipSetDevice(device));
    Stream stream;  // (destroyed after the events)
    Events<6> ev;
    HIP_TRY(stream.create());
    HIP_TRY(ev.create());
    cx.stream = stream.s;
    HIP_TRY(hipEventRecord(ev[0], cx.stream));

    // grouped order: a stable sort of the row indices by protein id (ignored rows, 0xFFFFFFFF, go last)
    DevBuf<uint32_t> key_in, key_out, row_in, row;
    DevBuf<unsigned char> sort_tmp;
    DevBuf<double> areas, L;
    DevBuf<uint64_t> d_off;
    HIP_TRY(key_in.alloc(n_rows));
    HIP_TRY(key_out.alloc(n_rows));
    HIP_TRY(row_in.alloc(n_rows));
    HIP_TRY(row.alloc(n_rows));
    HIP_TRY(hipMemcpyAsync(key_in.p, in.protein_of_row, (size_t)n_rows * 4, hipMemcpyHostToDevice, cx.stream));
    hipLaunchKernelGGL(plfq_iota_kernel, dim3((n_rows + PLFQ_THREADS - 1) / PLFQ_THREADS), dim3(PLFQ_THREADS), 0, cx.stream, n_rows, row_in.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(with_scratch(sort_tmp, [&](void* t, size_t& b) {
        return rocprim::radix_sort_pairs(t, b, key_in.p, key_out.p, row_in.p, row.p, (size_t)n_rows, 0, 32, cx.stream);
    }));
    HIP_TRY(d_off.alloc((size_t)NP + 1));
    HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), ((size_t)NP + 1) * 8, hipMemcpyHostToDevice, cx.stream));
    HIP_TRY(areas.alloc((size_t)n_rows * n));
    HIP_TRY(L.alloc((size_t)n_used * n));
    const uint64_t n_cells = n_used * n;
    if (n_cells) {
        HIP_TRY(hipMemcpyAsync(areas.p, in.areas, (size_t)n_rows * n * 8, hipMemcpyHostToDevice, cx.stream));
        const uint64_t blocks = (n_cells + PLFQ_THREADS - 1) / PLFQ_THREADS;
        if (blocks >= (1ull << 31)) return cx.fail(SAGE_HIP_ERR_UNSUPPORTED, "sage_hip_protein_lfq: more than 2^39 cells");
        hipLaunchKernelGGL(plfq_log_kernel, dim3((uint32_t)blocks), dim3(PLFQ_THREADS), 0, cx.stream, (uint32_t)n_used, n, areas.p, row.p, L.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[1], cx.stream));
    HIP_TRY(hipStreamSynchronize(cx.stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    out.log_ms = ms;
    out.device_ms = ms;

    // batches: what one protein holds on the device, and the solve kernel's workspace
    const double budget = workspace_budget_bytes();
    const uint64_t matrix_bytes = ((uint64_t)n * (n + 1) + n) * 8;
    const bool in_lds = matrix_bytes <= PLFQ_LDS_BYTES;
    const double per_protein = (double)P * 12.0 + (double)n * 32.0 + 8.0;
    uint32_t slots = PLFQ_MAX_SLOTS;
    if (!in_lds) slots = (uint32_t)std::min<double>(PLFQ_MAX_SLOTS, std::max(1.0, std::floor(budget * 0.5 / (double)matrix_bytes)));
    slots = std::min(slots, NP);
    const double left = budget - (in_lds ? 0.0 : (double)slots * (double)matrix_bytes);
    const uint32_t slices = (uint32_t)((P + PLFQ_PAIRS_PER_BLOCK - 1) / PLFQ_PAIRS_PER_BLOCK);
    uint64_t batch = (uint64_t)std::min<double>((double)NP, std::max(1.0, std::floor(left / per_protein)));
    if (slices) batch = std::min<uint64_t>(batch, std::max<uint64_t>(1, ((1ull << 31) - 1) / slices));
    DevBuf<double> ws, med, col, logab, inten;
    DevBuf<uint32_t> cnt, ncol, comp, nrows, ncomp, bad, long_list;
    std::vector<uint32_t> longs;
    const uint32_t long_slices = (uint32_t)((P + PLFQ_WAVES - 1) / PLFQ_WAVES);
    if (long_slices) batch = std::min<uint64_t>(batch, std::max<uint64_t>(1, ((1ull << 31) - 1) / long_slices));
    if (!in_lds) HIP_TRY(ws.alloc((size_t)slots * (matrix_bytes / 8)));
    HIP_TRY(med.alloc((size_t)batch * P));
    HIP_TRY(cnt.alloc((size_t)batch * P));
    HIP_TRY(col.alloc((size_t)batch * n));
    HIP_TRY(ncol.alloc((size_t)batch * n));
    HIP_TRY(logab.alloc((size_t)batch * n));
    HIP_TRY(inten.alloc((size_t)batch * n));
    HIP_TRY(comp.alloc((size_t)batch * n));
    HIP_TRY(nrows.alloc(batch));
    HIP_TRY(ncomp.alloc(batch));
    HIP_TRY(bad.alloc(1));
    HIP_TRY(hipMemsetAsync(bad.p, 0, 4, cx.stream));
    for (uint64_t first = 0; first < NP; first += batch) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(batch, NP - first);
        HIP_TRY(hipEventRecord(ev[2], cx.stream));
        if (slices) {
            hipLaunchKernelGGL(plfq_pair_median_kernel, dim3(nb * slices), dim3(PLFQ_THREADS), 0, cx.stream, L.p, n_used, d_off.p, (uint32_t)first,
                               n, slices, mc, med.p, cnt.p, (const uint32_t*)nullptr, PLFQ_PAIRS_PER_WAVE);
            HIP_TRY(hipGetLastError());
            longs.clear();
            for (uint32_t lp = 0; lp < nb; ++lp)
                if (off[first + lp + 1] - off[first + lp] > PLFQ_LDS_KEYS) longs.push_back(lp);
            if (!longs.empty()) {
                HIP_TRY(long_list.reserve(longs.size()));
                HIP_TRY(hipMemcpyAsync(long_list.p, longs.data(), longs.size() * 4, hipMemcpyHostToDevice, cx.stream));
                hipLaunchKernelGGL(plfq_pair_median_kernel, dim3((uint32_t)longs.size() * long_slices), dim3(PLFQ_THREADS), 0, cx.stream, L.p,
                                   n_used, d_off.p, (uint32_t)first, n, long_slices, mc, med.p, cnt.p, (const uint32_t*)long_list.p, 1u);
                HIP_TRY(hipGetLastError());
            }
        }
        HIP_TRY(hipEventRecord(ev[3], cx.stream));
        hipLaunchKernelGGL(plfq_solve_kernel, dim3(std::min(slots, nb)), dim3(PLFQ_THREADS), in_lds ? (size_t)matrix_bytes : 0, cx.stream, L.p,
                           n_used, d_off.p, (uint32_t)first, nb, n, mc, med.p, cnt.p, in_lds ? 1 : 0, ws.p, col.p, ncol.p, logab.p, inten.p,
                           comp.p, nrows.p, ncomp.p, bad.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[4], cx.stream));
        const size_t o = (size_t)first * n, cells = (size_t)nb * n;
        if (cells) {
            HIP_TRY(hipMemcpyAsync(out.log_abundance + o, logab.p, cells * 8, hipMemcpyDeviceToHost, cx.stream));
            HIP_TRY(hipMemcpyAsync(out.intensity + o, inten.p, cells * 8, hipMemcpyDeviceToHost, cx.stream));
            HIP_TRY(hipMemcpyAsync(out.component + o, comp.p, cells * 4, hipMemcpyDeviceToHost, cx.stream));
        }
        HIP_TRY(hipMemcpyAsync(out.n_rows_used + first, nrows.p, (size_t)nb * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(out.n_components + first, ncomp.p, (size_t)nb * 4, hipMemcpyDeviceToHost, cx.stream));
        if (P && out.pair_median) HIP_TRY(hipMemcpyAsync(out.pair_median + first * P, med.p, (size_t)nb * P * 8, hipMemcpyDeviceToHost, cx.stream));
        if (P && out.pair_count) HIP_TRY(hipMemcpyAsync(out.pair_count + first * P, cnt.p, (size_t)nb * P * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipEventRecord(ev[5], cx.stream));
        HIP_TRY(hipStreamSynchronize(cx.stream));
        HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[3]));
        out.median_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, ev[3], ev[4]));
        out.solve_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[5]));
        out.device_ms += ms;
        ++out.n_batches;
    }
    uint32_t bad_host = 0;
    HIP_TRY(hipMemcpy(&bad_host, bad.p, 4, hipMemcpyDeviceToHost));
    if (bad_host)
        return cx.fail(SAGE_HIP_ERR_INTERNAL, "sage_hip_protein_lfq: a zero or non-finite pivot in the normal equations of protein " +
                                                  std::to_string(bad_host - 1));
    return true;
}

}  // namespace

int protein_lfq_on_device(int device, const SageProteinLfqInput& in, SageProteinLfqOutput& out, std::string& err) {
    Ctx cx;
    cx.prefix = "sage_hip_protein_lfq: ";
    if (protein_lfq_impl(cx, device, in, out)) return SAGE_HIP_OK;
    err = cx.err;
    return cx.code;
}

}  // namespace sagehip
