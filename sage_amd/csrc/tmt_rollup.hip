// tmt_rollup.hip — the roll-up of TMT reporter intensities to one abundance per group (protein, peptide) and channel on the device
// (DESIGN.md 7i): which rows are used, the column sums and loading factors, then per group and channel the sum of the weighted cells
// or the median of their centred logs.  The arithmetic is tmt_rollup.h's, which the host emulation shares.
//
//   tmtr_row_kernel       a team of T lanes (T: the power of two that holds the channels, at most 64) per input row: the present
//                         cells of the row by a butterfly sum of integers; key[r] = the row's group when it is used, else 0xFFFFFFFF;
//                         the used rows of every group by integer atomics.  The rows are then grouped by a stable radix sort of the
//                         keys (rocPRIM), so a group's used rows are one range of the grouped order, in ascending row index.
//   tmtr_partial_kernel   block b of 1 024 input rows, one thread per channel walking the rows in order: loads coalesced across the
//                         channels, P[b][k] and the block's count of present cells.
//   tmtr_fold_kernel      one workgroup: S[k] and C[k] from the partials in ascending b, one thread per channel; M by one thread in
//                         ascending k; the factors.
//   tmtr_sum_kernel       (Sum) one wavefront per group, lanes over the channels in slabs of 64: the rows of the group in order (64
//                         row indices loaded at once, handed round by shuffles), every lane its own chain of additions.
//   tmtr_centre_kernel    (Median) one thread per used row in grouped order: the logs of its cells, its centre, and the centred
//                         logs d into a channel-major table D[k][grouped row] (NaN: missing), so a (group, channel) is one
//                         contiguous stream.
//   tmtr_group_centre_kernel  a[g], one thread per group over the centres of its rows in order.
//   tmtr_median_kernel    (Median) one wavefront per (group, few channels): the keys of the present d (maxlfq::key_of) compacted by
//                         ballot into the wave's LDS slice while the group has at most TMTR_LDS_KEYS rows; the two ranks selected
//                         exactly and wave-uniformly: up to 64 keys one per lane by counting with ballots, beyond that by
//                         maxlfq::radix_select over the LDS slice, or — a longer group — over the column read again (those groups in
//                         a launch of their own, one channel per wavefront).
// No floating-point atomics, nothing that depends on arrival order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <rocprim/device/device_radix_sort.hpp>

#include "device_types.h"
#include "hip_host.h"
#include "tmt_rollup.h"

namespace sagehip {

namespace {

constexpr uint32_t TMTR_THREADS = 256;
constexpr uint32_t TMTR_WAVES = TMTR_THREADS / 64;
constexpr uint32_t TMTR_LDS_KEYS = 1024;          // keys a wavefront stages in LDS (8 KB per wave, 32 KB per workgroup)
constexpr uint32_t TMTR_CHANNELS_PER_WAVE = 8;    // consecutive channels one wavefront works through
constexpr uint32_t TMTR_CHANNELS_PER_BLOCK = TMTR_WAVES * TMTR_CHANNELS_PER_WAVE;
constexpr uint32_t TMTR_PARTIAL_THREADS = 64;

__global__ __launch_bounds__(TMTR_THREADS) void tmtr_iota_kernel(uint32_t n, uint32_t* out) {
    const uint32_t i = blockIdx.x * TMTR_THREADS + threadIdx.x;
    if (i < n) out[i] = i;
}

// team: lanes of one row (a power of two, <= 64; 256 is a multiple, so a team never straddles a wavefront)
__global__ __launch_bounds__(TMTR_THREADS) void tmtr_row_kernel(uint32_t n_rows, uint32_t n_labels, uint32_t team, uint32_t need,
                                                                 const float* __restrict__ intensity, const uint32_t* __restrict__ group,
                                                                 uint32_t* __restrict__ key, uint32_t* __restrict__ count) {
    const uint64_t t = (uint64_t)blockIdx.x * TMTR_THREADS + threadIdx.x;
    const uint64_t r = t / team;
    const uint32_t lane = (uint32_t)(t % team);
    uint32_t c = 0;
    if (r < n_rows) {
        const float* row = intensity + r * n_labels;
        for (uint32_t k = lane; k < n_labels; k += team) c += tmtroll::present(row[k]) ? 1u : 0u;
    }
    for (uint32_t o = team >> 1; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, (int)o);  // (every lane of the wavefront takes part)
    if (r < n_rows && lane == 0) {
        const uint32_t g = group[r];
        const bool used = g != tmtroll::NONE && c >= need;
        key[r] = used ? g : tmtroll::NONE;
        if (used) atomicAdd(count + g, 1u);
    }
}

__global__ __launch_bounds__(TMTR_PARTIAL_THREADS) void tmtr_partial_kernel(uint32_t n_rows, uint32_t n_labels,
                                                                             const float* __restrict__ intensity,
                                                                             const uint32_t* __restrict__ key, double* __restrict__ P,
                                                                             uint32_t* __restrict__ PC) {
    const uint32_t b = blockIdx.x, k = blockIdx.y * TMTR_PARTIAL_THREADS + threadIdx.x;
    if (k >= n_labels) return;
    const uint64_t lo = (uint64_t)b * tmtroll::BLOCK_ROWS;
    const uint64_t hi = lo + tmtroll::BLOCK_ROWS < n_rows ? lo + tmtroll::BLOCK_ROWS : n_rows;
    const uint64_t o = (uint64_t)b * n_labels + k;
    tmtroll::block_partial(intensity, n_labels, k, lo, hi, [&](uint64_t r) { return key[r] != tmtroll::NONE; }, P + o, PC + o);
}

__global__ __launch_bounds__(TMTR_THREADS) void tmtr_fold_kernel(uint32_t n_blocks, uint32_t n_labels, int normalise,
                                                                  const double* __restrict__ P, const uint32_t* __restrict__ PC,
                                                                  double* __restrict__ S, uint32_t* __restrict__ C, double* __restrict__ f) {
    __shared__ double M;
    for (uint32_t k = threadIdx.x; k < n_labels; k += TMTR_THREADS) tmtroll::fold_partials(P, PC, n_blocks, n_labels, k, S + k, C + k);
    __syncthreads();
    if (threadIdx.x == 0) M = tmtroll::mean_column_sum(S, C, n_labels);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n_labels; k += TMTR_THREADS) f[k] = tmtroll::factor_of(normalise, M, S[k], C[k]);
}

// LDS writes of some lanes of a wavefront, read by others of the same wavefront afterwards
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// off: the range of every group in grouped order; row: the input row of every position of the grouped order
__global__ __launch_bounds__(TMTR_THREADS) void tmtr_sum_kernel(uint32_t n_groups, uint32_t n_labels, const uint64_t* __restrict__ off,
                                                                 const uint32_t* __restrict__ row, const float* __restrict__ intensity,
                                                                 const double* __restrict__ f, double* __restrict__ abundance,
                                                                 double* __restrict__ log_abundance, uint32_t* __restrict__ n_cells) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t g = (uint64_t)blockIdx.x * TMTR_WAVES + (threadIdx.x >> 6);
    if (g >= n_groups) return;  // (wave-uniform)
    const uint64_t a = off[g];
    const uint32_t nr = (uint32_t)(off[g + 1] - a);
    for (uint32_t k0 = 0; k0 < n_labels; k0 += 64) {
        const uint32_t k = k0 + lane;
        const bool active = k < n_labels;
        const double fk = active ? f[k] : 1.0;
        double s = 0.0;
        uint32_t c = 0;
        for (uint32_t base = 0; base < nr; base += 64) {
            const uint32_t mine = base + lane < nr ? row[a + base + lane] : 0u;
            const uint32_t m = nr - base < 64u ? nr - base : 64u;
            for (uint32_t i = 0; i < m; ++i) {
                const uint32_t r = (uint32_t)__shfl((int)mine, (int)i);
                if (active) {
                    const float x = intensity[(uint64_t)r * n_labels + k];
                    if (tmtroll::present(x)) {
                        s = s + tmtroll::weighted(x, fk);
                        ++c;
                    }
                }
            }
        }
        if (active) {
            const uint64_t o = g * n_labels + k;
            tmtroll::finish_sum(s, c, abundance + o, log_abundance + o);
            n_cells[o] = c;
        }
    }
}

// D[k * n_used + i] for the i-th row of the grouped order, i < n_used; centre[i]
__global__ __launch_bounds__(TMTR_THREADS) void tmtr_centre_kernel(uint32_t n_used, uint32_t n_labels, const uint32_t* __restrict__ row,
                                                                    const float* __restrict__ intensity, const double* __restrict__ f,
                                                                    double* __restrict__ D, double* __restrict__ centre) {
    const uint32_t i = blockIdx.x * TMTR_THREADS + threadIdx.x;
    if (i >= n_used) return;
    const float* cells = intensity + (uint64_t)row[i] * n_labels;
    const double c = tmtroll::row_centre(cells, f, n_labels, [&](uint32_t k, double l) { D[(uint64_t)k * n_used + i] = l; });
    centre[i] = c;
    for (uint32_t k = 0; k < n_labels; ++k) {
        double* d = D + (uint64_t)k * n_used + i;
        *d = *d - c;  // (missing stays NaN)
    }
}

__global__ __launch_bounds__(TMTR_THREADS) void tmtr_group_centre_kernel(uint32_t n_groups, const uint64_t* __restrict__ off,
                                                                          const double* __restrict__ centre, double* __restrict__ a) {
    const uint32_t g = blockIdx.x * TMTR_THREADS + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t nr = (uint32_t)(off[g + 1] - off[g]);
    a[g] = nr ? tmtroll::group_centre(centre + off[g], nr) : maxlfq::missing();
}

// Groups first .. first + gridDim.x / slices.  Two launches: without long_list every group, channels_per_wave consecutive channels
// per wavefront, where a group of more than TMTR_LDS_KEYS rows is passed over; with long_list (exactly those groups) one channel per
// wavefront, since each of their channels costs up to 128 passes over its column.
__global__ __launch_bounds__(TMTR_THREADS) void tmtr_median_kernel(const double* __restrict__ D, uint64_t n_used, const uint64_t* __restrict__ off,
                                                                    uint32_t first, uint32_t n_labels, uint32_t slices,
                                                                    const double* __restrict__ centre_of_group, double* __restrict__ abundance,
                                                                    double* __restrict__ log_abundance, uint32_t* __restrict__ n_cells,
                                                                    const uint32_t* __restrict__ long_list, uint32_t channels_per_wave) {
    __shared__ uint64_t lds_keys[TMTR_WAVES][TMTR_LDS_KEYS];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t g = long_list ? long_list[first + blockIdx.x / slices] : first + blockIdx.x / slices, slice = blockIdx.x % slices;
    uint32_t q = (slice * TMTR_WAVES + w) * channels_per_wave;
    if (q >= n_labels) return;  // (wave-uniform: there is no workgroup barrier below)
    const uint64_t a = off[g];
    const uint32_t nr = (uint32_t)(off[g + 1] - a);
    const bool staged = nr <= TMTR_LDS_KEYS;
    if (staged != (long_list == nullptr)) return;  // a long group's channels belong to the launch over long_list
    uint64_t* keys = lds_keys[w];
    const double ag = centre_of_group[g];
    for (uint32_t step = 0; step < channels_per_wave && q < n_labels; ++step, ++q) {
        const double* col = D + (uint64_t)q * n_used + a;
        uint32_t c = 0;
        for (uint32_t base = 0; base < nr; base += 64) {
            const uint32_t r = base + lane;
            const double d = r < nr ? col[r] : maxlfq::missing();
            const bool here = maxlfq::present(d);
            const uint64_t mask = __ballot(here);
            if (staged && here) keys[c + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = maxlfq::key_of(d);
            c += (uint32_t)__popcll(mask);
        }
        wave_sync();
        uint64_t klo = 0, khi = 0;
        if (c) {  // (wave-uniform)
            const uint32_t rank_lo = (c - 1) / 2, rank_hi = c / 2;
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
                        const double d = r < nr ? col[r] : maxlfq::missing();
                        z += wave_count(maxlfq::present(d) && (maxlfq::key_of(d) >> bit) == (prefix >> bit));
                    }
                    return z;
                };
                klo = maxlfq::radix_select(rank_lo, zeros);
                khi = rank_hi == rank_lo ? klo : maxlfq::radix_select(rank_hi, zeros);
            }
        }
        if (lane == 0) {
            const uint64_t o = (uint64_t)g * n_labels + q;
            tmtroll::finish_median(klo, khi, c, ag, abundance + o, log_abundance + o);
            n_cells[o] = c;
        }
        wave_sync();  // (the next channel writes the keys again)
    }
}

uint32_t team_of(uint32_t n_labels) {
    uint32_t t = 1;
    while (t < n_labels && t < 64) t <<= 1;
    return t;
}

bool tmt_rollup_impl(Ctx& cx, const SageTmtRollupInput& in, SageTmtRollupOutput& out) {
    const uint32_t n = in.n_labels, NG = in.n_groups;
    const uint32_t n_rows = (uint32_t)in.n_rows;  // (< 2^31: the entry point's guard)
    const uint32_t n_blocks = (n_rows + tmtroll::BLOCK_ROWS - 1) / tmtroll::BLOCK_ROWS;
    const uint32_t team = team_of(n);
    const size_t cells_in = (size_t)n_rows * n, cells_out = (size_t)NG * n;

    Events<5> ev;
    HIP_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev[0], cx.stream));
    DevBuf<float> intensity;
    DevBuf<uint32_t> group, key, key_sorted, row_in, row, count, PC, C;
    DevBuf<unsigned char> sort_tmp;
    DevBuf<double> P, S, f;
    HIP_TRY(intensity.alloc(cells_in));
    HIP_TRY(group.alloc(n_rows));
    HIP_TRY(key.alloc(n_rows));
    HIP_TRY(key_sorted.alloc(n_rows));
    HIP_TRY(row_in.alloc(n_rows));
    HIP_TRY(row.alloc(n_rows));
    HIP_TRY(count.alloc(NG));
    HIP_TRY(P.alloc((size_t)n_blocks * n));
    HIP_TRY(PC.alloc((size_t)n_blocks * n));
    HIP_TRY(S.alloc(n));
    HIP_TRY(C.alloc(n));
    HIP_TRY(f.alloc(n));
    HIP_TRY(hipMemcpyAsync(intensity.p, in.intensity, cells_in * 4, hipMemcpyHostToDevice, cx.stream));
    HIP_TRY(hipMemcpyAsync(group.p, in.group_of_row, (size_t)n_rows * 4, hipMemcpyHostToDevice, cx.stream));
    HIP_TRY(hipMemsetAsync(count.p, 0, (size_t)NG * 4, cx.stream));
    const uint64_t row_blocks = ((uint64_t)n_rows * team + TMTR_THREADS - 1) / TMTR_THREADS;  // (< 2^29)
    hipLaunchKernelGGL(tmtr_row_kernel, dim3((uint32_t)row_blocks), dim3(TMTR_THREADS), 0, cx.stream, n_rows, n, team,
                       tmtroll::needed(in.min_present), intensity.p, group.p, key.p, count.p);
    HIP_TRY(hipGetLastError());
    // grouped order: a stable sort of the row indices by key (rows that are not used, 0xFFFFFFFF, go last)
    hipLaunchKernelGGL(tmtr_iota_kernel, dim3((n_rows + TMTR_THREADS - 1) / TMTR_THREADS), dim3(TMTR_THREADS), 0, cx.stream, n_rows, row_in.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(with_scratch(sort_tmp, [&](void* t, size_t& b) {
        return rocprim::radix_sort_pairs(t, b, key.p, key_sorted.p, row_in.p, row.p, (size_t)n_rows, 0, 32, cx.stream);
    }));
    hipLaunchKernelGGL(tmtr_partial_kernel, dim3(n_blocks, (n + TMTR_PARTIAL_THREADS - 1) / TMTR_PARTIAL_THREADS), dim3(TMTR_PARTIAL_THREADS), 0,
                       cx.stream, n_rows, n, intensity.p, key.p, P.p, PC.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tmtr_fold_kernel, dim3(1), dim3(TMTR_THREADS), 0, cx.stream, n_blocks, n, (int)in.normalise, P.p, PC.p, S.p, C.p, f.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out.n_rows_used, count.p, (size_t)NG * 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(out.factor, f.p, (size_t)n * 8, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(out.column_sum, S.p, (size_t)n * 8, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipEventRecord(ev[1], cx.stream));
    HIP_TRY(hipStreamSynchronize(cx.stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    out.norm_ms = out.device_ms = ms;

    // the ranges of the groups in grouped order
    std::vector<uint64_t> off((size_t)NG + 1, 0);
    for (uint32_t g = 0; g < NG; ++g) off[(size_t)g + 1] = off[g] + out.n_rows_used[g];
    const uint64_t n_used = off[NG];
    out.n_used_rows = n_used;
    if (n_used == 0) {  // no summary launch: every group not quantified
        for (size_t i = 0; i < cells_out; ++i) {
            out.abundance[i] = 0.0;
            out.log_abundance[i] = std::nan("");
            out.n_cells[i] = 0;
        }
        return true;
    }
    out.n_label_slabs = (n + 63) / 64;
    DevBuf<uint64_t> d_off;
    DevBuf<double> ab, la, D, centre, a;
    DevBuf<uint32_t> nc, long_list;
    HIP_TRY(d_off.alloc((size_t)NG + 1));
    HIP_TRY(ab.alloc(cells_out));
    HIP_TRY(la.alloc(cells_out));
    HIP_TRY(nc.alloc(cells_out));
    HIP_TRY(hipEventRecord(ev[2], cx.stream));
    HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), ((size_t)NG + 1) * 8, hipMemcpyHostToDevice, cx.stream));
    if (in.summary == tmtroll::SUMMARY_SUM) {
        hipLaunchKernelGGL(tmtr_sum_kernel, dim3((NG + TMTR_WAVES - 1) / TMTR_WAVES), dim3(TMTR_THREADS), 0, cx.stream, NG, n, d_off.p, row.p,
                           intensity.p, f.p, ab.p, la.p, nc.p);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(D.alloc((size_t)n_used * n));
        HIP_TRY(centre.alloc(n_used));
        HIP_TRY(a.alloc(NG));
        hipLaunchKernelGGL(tmtr_centre_kernel, dim3((uint32_t)((n_used + TMTR_THREADS - 1) / TMTR_THREADS)), dim3(TMTR_THREADS), 0, cx.stream,
                           (uint32_t)n_used, n, row.p, intensity.p, f.p, D.p, centre.p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(tmtr_group_centre_kernel, dim3((NG + TMTR_THREADS - 1) / TMTR_THREADS), dim3(TMTR_THREADS), 0, cx.stream, NG, d_off.p,
                           centre.p, a.p);
        HIP_TRY(hipGetLastError());
        // launches of at most 2^31 - 1 workgroups
        const uint32_t slices = (n + TMTR_CHANNELS_PER_BLOCK - 1) / TMTR_CHANNELS_PER_BLOCK, long_slices = (n + TMTR_WAVES - 1) / TMTR_WAVES;
        const uint32_t per_launch = ((1u << 31) - 1) / slices;
        for (uint64_t first = 0; first < NG; first += per_launch) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(per_launch, NG - first);
            hipLaunchKernelGGL(tmtr_median_kernel, dim3(nb * slices), dim3(TMTR_THREADS), 0, cx.stream, D.p, n_used, d_off.p, (uint32_t)first, n,
                               slices, a.p, ab.p, la.p, nc.p, (const uint32_t*)nullptr, TMTR_CHANNELS_PER_WAVE);
            HIP_TRY(hipGetLastError());
        }
        std::vector<uint32_t> longs;
        for (uint32_t g = 0; g < NG; ++g)
            if (out.n_rows_used[g] > TMTR_LDS_KEYS) longs.push_back(g);
        out.n_long_groups = (uint32_t)longs.size();
        if (!longs.empty()) {
            HIP_TRY(long_list.alloc(longs.size()));
            HIP_TRY(hipMemcpyAsync(long_list.p, longs.data(), longs.size() * 4, hipMemcpyHostToDevice, cx.stream));
            const uint32_t long_per_launch = ((1u << 31) - 1) / long_slices;
            for (uint64_t first = 0; first < longs.size(); first += long_per_launch) {
                const uint32_t nb = (uint32_t)std::min<uint64_t>(long_per_launch, longs.size() - first);
                hipLaunchKernelGGL(tmtr_median_kernel, dim3(nb * long_slices), dim3(TMTR_THREADS), 0, cx.stream, D.p, n_used, d_off.p,
                                   (uint32_t)first, n, long_slices, a.p, ab.p, la.p, nc.p, (const uint32_t*)long_list.p, 1u);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    HIP_TRY(hipEventRecord(ev[3], cx.stream));
    HIP_TRY(hipMemcpyAsync(out.abundance, ab.p, cells_out * 8, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(out.log_abundance, la.p, cells_out * 8, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(out.n_cells, nc.p, cells_out * 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipEventRecord(ev[4], cx.stream));
    HIP_TRY(hipStreamSynchronize(cx.stream));
    HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[3]));
    out.summary_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[4]));
    out.device_ms += ms;
    return true;
}

}  // namespace

int tmt_rollup_on_device(int device, const SageTmtRollupInput& in, SageTmtRollupOutput& out, std::string& err) {
    return run_on_device(device, "sage_hip_tmt_rollup", "sage_hip_tmt_rollup: ", err, [&](Ctx& cx) { return tmt_rollup_impl(cx, in, out); });
}

}  // namespace sagehip
