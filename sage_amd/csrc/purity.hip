// purity.hip — precursor purity of reported PSMs from MS1 scans on the device (sage_hip_precursor_purity; the definition is
// purity.h, the account DESIGN.md 7h).  An addition over the reference.
//
// Work unit: one MS1 spectrum with all the queries that name it — one workgroup of 4 wavefronts, the queries dealt to the
// wavefronts in turn.  The host groups the queries by spectrum (a stable counting sort, so a unit's queries keep their order),
// streams the MS1 batches through the device one at a time with the queries of that batch, and scatters the results back to
// the queries' own positions.
//
// Two routes, per spectrum, by a flag that sorted_flag_kernel computes ("m/z non-decreasing and NaN-free"):
//   sorted  the window and the `below` interval are found by wave-wide partition points (the idiom of kernels.hip's
//           wave_partition_point) and only their peaks are read; each of the window's peaks is tested against the envelope.
//   scan    any order: the spectrum passes through LDS in position-ordered chunks of PUR_CHUNK peaks (any number of chunks, so a
//           spectrum beyond a compute unit's LDS is the same code path); each wavefront tests 64 peaks at a time for each of its
//           queries.  Between chunks a query's sums and counts rest in its own output cells.
// On both routes the hits of 64 peaks are compacted by ballot, which keeps position order, and the f64 sums are added hit
// after hit in that order by a wave-uniform loop (every lane adds the same broadcast value): no tree, no per-lane partial sum.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "core.h"
#include "device_types.h"
#include "hip_host.h"
#include "purity.h"

namespace sagehip {

namespace {

constexpr int PUR_WAVES = 4;                  // wavefronts per workgroup (one MS1 spectrum)
constexpr int PUR_THREADS = 64 * PUR_WAVES;
constexpr uint32_t PUR_CHUNK = 2048;          // peaks of one LDS chunk of the scan route (16 KB)

__device__ __forceinline__ float bcast(float v, uint32_t lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)lane));
}

// the first index in [lo, hi) of non-decreasing, NaN-free m[] that is not below v (STRICT: m[i] < v) / not at or below v
template <bool STRICT>
__device__ __forceinline__ uint32_t wave_lower(const float* __restrict__ m, uint32_t lo, uint32_t hi, float v, uint32_t lane) {
    while (hi - lo > 64u) {
        // 64 pivots `step` apart with 64 * step >= span; the answer lies in [lo + c * step, lo + (c + 1) * step - 1] after c of them
        // compare true, which is shorter than the span
        const uint32_t step = (hi - lo + 63u) / 64u;
        const uint64_t idx = (uint64_t)lo + (uint64_t)(lane + 1u) * step - 1u;
        bool t = false;
        if (idx < hi) {
            const float x = m[idx];
            t = STRICT ? x < v : x <= v;
        }
        const uint32_t c = (uint32_t)__popcll(__ballot(t));
        const uint64_t nhi = (uint64_t)lo + (uint64_t)(c + 1u) * step - 1u;
        hi = nhi < hi ? (uint32_t)nhi : hi;
        lo = lo + c * step < hi ? lo + c * step : hi;  // (already so on input that keeps the precondition; never past the end on any)
    }
    bool t = false;
    if (lo + lane < hi) {
        const float x = m[lo + lane];
        t = STRICT ? x < v : x <= v;
    }
    return lo + (uint32_t)__popcll(__ballot(t));
}
// [first, end) of the peaks inside [lo, hi] (lo <= hi); the end is looked for next to the first before the rest of the spectrum
__device__ __forceinline__ void wave_interval(const float* __restrict__ m, uint32_t n, float lo, float hi, uint32_t lane, uint32_t& first,
                                              uint32_t& end) {
    first = wave_lower<true>(m, 0, n, lo, lane);
    const uint32_t near = n - first < 64u ? n : first + 64u;
    end = wave_lower<false>(m, first, near, hi, lane);
    if (end == near && near < n) end = wave_lower<false>(m, near, n, hi, lane);
}

struct Bounds {          // of one query: uniform over the wavefront but for (elo, ehi), the envelope bounds of the LANE's own k
    float wlo, whi, blo, bhi, elo, ehi;
};
struct Acc {             // uniform over the wavefront
    uint32_t n_window, n_matched;
    double total, matched, below;
};

// 64 peaks, one per lane (valid: the lane has one): their hits by ballot, then the sums hit after hit in position order
template <bool WINDOW, bool BELOW>
__device__ __forceinline__ void add64(const Bounds& b, uint32_t max_isotope, bool valid, float p, float it, Acc& acc) {
    uint64_t in_w = 0, in_m = 0, in_b = 0;
    if (WINDOW) {
        const bool w = valid && purity::inside(b.wlo, b.whi, p);
        in_w = __ballot(w);
        if (in_w) {
            bool hit = false;
            for (uint32_t k = 0; k <= max_isotope; ++k) {  // (uniform trip count: the broadcasts run with every lane converged)
                const float elo = bcast(b.elo, k), ehi = bcast(b.ehi, k);
                hit = hit | purity::inside(elo, ehi, p);
            }
            in_m = __ballot(w && hit);
        }
    }
    if (BELOW) in_b = __ballot(valid && purity::inside(b.blo, b.bhi, p));
    acc.n_window += (uint32_t)__popcll(in_w);
    acc.n_matched += (uint32_t)__popcll(in_m);
    uint64_t any = in_w | in_b;
    while (any) {
        const uint32_t j = (uint32_t)__builtin_ctzll(any);
        any &= any - 1;
        const double v = (double)bcast(it, j);
        if ((in_w >> j) & 1u) acc.total += v;
        if ((in_m >> j) & 1u) acc.matched += v;
        if ((in_b >> j) & 1u) acc.below += v;
    }
}

struct Queries {         // grouped by unit; results at the same positions
    const float* mz;
    const uint8_t* charge;
    const float *lo, *hi;
    uint32_t *n_window, *n_matched;
    double *total, *matched, *below;
    float* purity;
};

__device__ __forceinline__ Bounds bounds_of(const Queries& q, uint64_t g, const purity::Settings& st, uint32_t lane) {
    const float mz = q.mz[g];
    const uint32_t z = q.charge[g];
    Bounds b;
    purity::window_bounds(mz, q.lo[g], q.hi[g], st, b.wlo, b.whi);
    purity::below_bounds(mz, z, st, b.blo, b.bhi);
    purity::envelope_bounds(mz, z, lane, st, b.elo, b.ehi);  // (NaN bounds beyond max_isotope)
    return b;
}
__device__ __forceinline__ void store(const Queries& q, uint64_t g, const Acc& acc, bool last, uint32_t lane) {
    if (lane) return;
    purity::Result r{acc.n_window, acc.n_matched, acc.total, acc.matched, acc.below, 0.0f};
    if (last) r = purity::finish(acc.n_window, acc.n_matched, acc.total, acc.matched, acc.below);
    q.n_window[g] = r.n_window;
    q.n_matched[g] = r.n_matched;
    q.total[g] = r.total;
    q.matched[g] = r.matched;
    q.below[g] = r.below;
    if (last) q.purity[g] = r.purity;
}

// sorted[u] = the unit's spectrum has non-decreasing m/z without a NaN; one wavefront per unit
__global__ __launch_bounds__(PUR_THREADS) void sorted_flag_kernel(uint32_t n_units, const uint32_t* __restrict__ unit_spec,
                                                                   const uint64_t* __restrict__ off, const float* __restrict__ mz,
                                                                   uint8_t* __restrict__ sorted) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t u = (uint64_t)blockIdx.x * PUR_WAVES + (threadIdx.x >> 6);
    if (u >= n_units) return;  // (wave-uniform: no workgroup barrier below)
    const uint64_t a = off[unit_spec[u]], e = off[unit_spec[u] + 1];
    bool bad = false;
    for (uint64_t i = a + lane; i < e; i += 64) {
        const float x = mz[i], y = i + 1 < e ? mz[i + 1] : x;
        bad = bad || !(x <= y);  // (a NaN on either side, the single peak's own included)
    }
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0) sorted[u] = any_bad ? 0 : 1;
}

__global__ __launch_bounds__(PUR_THREADS) void purity_kernel(const uint32_t* __restrict__ unit_spec, const uint32_t* __restrict__ unit_qoff,
                                                              const uint8_t* __restrict__ sorted, int force_scan,
                                                              const uint64_t* __restrict__ off, const float* __restrict__ mz,
                                                              const float* __restrict__ inten, Queries q, purity::Settings st) {
    __shared__ __attribute__((aligned(16))) float s_mz[PUR_CHUNK];
    __shared__ __attribute__((aligned(16))) float s_in[PUR_CHUNK];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t u = blockIdx.x;
    const uint32_t q0 = unit_qoff[u], q1 = unit_qoff[u + 1];
    const uint64_t a = off[unit_spec[u]], e = off[unit_spec[u] + 1];
    if (sorted[u] && !force_scan) {
        const uint32_t n = (uint32_t)(e - a);
        const float* __restrict__ m = mz + a;
        const float* __restrict__ in = inten + a;
        for (uint32_t g = q0 + wave; g < q1; g += PUR_WAVES) {
            const Bounds b = bounds_of(q, g, st, lane);
            Acc acc{0u, 0u, 0.0, 0.0, 0.0};
            uint32_t first, end;
            if (b.wlo <= b.whi) {  // (else, a NaN bound included, no peak is inside)
                wave_interval(m, n, b.wlo, b.whi, lane, first, end);
                for (uint32_t base = first; base < end; base += 64) {
                    const bool valid = base + lane < end;
                    add64<true, false>(b, st.max_isotope, valid, valid ? m[base + lane] : 0.0f, valid ? in[base + lane] : 0.0f, acc);
                }
            }
            if (b.blo <= b.bhi) {
                wave_interval(m, n, b.blo, b.bhi, lane, first, end);
                for (uint32_t base = first; base < end; base += 64) {
                    const bool valid = base + lane < end;
                    add64<false, true>(b, st.max_isotope, valid, valid ? m[base + lane] : 0.0f, valid ? in[base + lane] : 0.0f, acc);
                }
            }
            store(q, g, acc, true, lane);
        }
        return;
    }
    // chunks of PUR_CHUNK peaks on 16-byte boundaries of the peak arrays: whole quads inside the spectrum are moved as float4
    const uint64_t g0 = a & ~(uint64_t)3;
    for (uint64_t cbase = g0; cbase == g0 || cbase < e; cbase += PUR_CHUNK) {  // (an empty spectrum: one empty chunk)
        __syncthreads();  // the chunk before is read; its results are stored
        for (uint32_t t = threadIdx.x * 4u; t < PUR_CHUNK; t += PUR_THREADS * 4u) {
            const uint64_t g = cbase + t;
            if (g >= e) break;
            if (g >= a && g + 4 <= e) {
                *reinterpret_cast<float4*>(s_mz + t) = *reinterpret_cast<const float4*>(mz + g);
                *reinterpret_cast<float4*>(s_in + t) = *reinterpret_cast<const float4*>(inten + g);
            } else {
                for (uint32_t j = 0; j < 4; ++j)
                    if (g + j >= a && g + j < e) {
                        s_mz[t + j] = mz[g + j];
                        s_in[t + j] = inten[g + j];
                    }
            }
        }
        __syncthreads();
        const uint32_t lo_i = a > cbase ? (uint32_t)(a - cbase) : 0u;
        const uint32_t hi_i = e - cbase < PUR_CHUNK ? (uint32_t)(e - cbase) : PUR_CHUNK;
        const bool first = cbase == g0, last = cbase + PUR_CHUNK >= e;
        for (uint32_t g = q0 + wave; g < q1; g += PUR_WAVES) {
            const Bounds b = bounds_of(q, g, st, lane);
            Acc acc{0u, 0u, 0.0, 0.0, 0.0};
            if (!first) acc = Acc{q.n_window[g], q.n_matched[g], q.total[g], q.matched[g], q.below[g]};
            for (uint32_t base = lo_i; base < hi_i; base += 64) {
                const bool valid = base + lane < hi_i;
                add64<true, true>(b, st.max_isotope, valid, valid ? s_mz[base + lane] : 0.0f, valid ? s_in[base + lane] : 0.0f, acc);
            }
            store(q, g, acc, last, lane);
        }
    }
}

template <class T>
void scatter(const std::vector<T>& from, const std::vector<uint64_t>& order, uint64_t first, T* to) {
    for (size_t i = 0; i < from.size(); ++i) to[order[first + i]] = from[i];
}

bool purity_impl(Ctx& cx, int device, const SagePurityInput& in, SagePurityOutput& out) {
    const SagePuritySettings& s = in.settings;
    const purity::Settings st{s.ppm_tolerance, s.default_isolation_lo, s.default_isolation_hi, s.max_isotope};
    const char* knob = std::getenv("SAGE_HIP_PURITY_SCAN");  // read once per call
    const int force_scan = knob && *knob && std::strcmp(knob, "0") != 0;
    // spectra are numbered through the batches in order; the queries grouped by spectrum, stably
    std::vector<uint64_t> batch_first((size_t)in.n_ms1 + 1, 0);
    for (uint32_t b = 0; b < in.n_ms1; ++b) batch_first[b + 1] = batch_first[b] + in.ms1[b].n_spectra;
    const uint64_t n_spectra = batch_first[in.n_ms1];
    std::vector<uint64_t> q_off((size_t)n_spectra + 1, 0);
    for (uint64_t i = 0; i < in.n_queries; ++i)
        if (in.ms1_index[i] != purity::NO_MS1) ++q_off[in.ms1_index[i] + 1];
    for (uint64_t sp = 0; sp < n_spectra; ++sp) q_off[sp + 1] += q_off[sp];
    std::vector<uint64_t> order(q_off[n_spectra]);
    {
        std::vector<uint64_t> next(q_off.begin(), q_off.end() - 1);
        for (uint64_t i = 0; i < in.n_queries; ++i) {
            const uint64_t sp = in.ms1_index[i];
            if (sp != purity::NO_MS1) {
                order[next[sp]++] = i;
                continue;
            }
            const purity::Result none = purity::no_result();
            out.n_window[i] = none.n_window;
            out.n_matched[i] = none.n_matched;
            out.total[i] = none.total;
            out.matched[i] = none.matched;
            out.below[i] = none.below;
            out.purity[i] = none.purity;
        }
    }
    if (order.empty()) return true;
    HIP_TRY(hipSetDevice(device));
    Stream stream;  // (destroyed after the events)
    Events<4> ev;
    HIP_TRY(stream.create());
    HIP_TRY(ev.create());
    cx.stream = stream.s;
    DevBuf<uint64_t> d_off;
    DevBuf<float> d_mz, d_in, d_qmz, d_qlo, d_qhi, d_pur;
    DevBuf<uint8_t> d_qz, d_sorted;
    DevBuf<uint32_t> d_spec, d_qoff, d_nw, d_nm;
    DevBuf<double> d_tot, d_mat, d_bel;
    std::vector<uint32_t> unit_spec, unit_qoff, h_nw, h_nm;
    std::vector<float> qmz, qlo, qhi, h_pur;
    std::vector<uint8_t> qz, h_sorted;
    std::vector<double> h_tot, h_mat, h_bel;
    const float nan = std::nanf("");
    for (uint32_t b = 0; b < in.n_ms1; ++b) {
        const SageRawBatch& r = in.ms1[b];
        const uint64_t s0 = batch_first[b], s1 = batch_first[b + 1], first = q_off[s0], nq = q_off[s1] - first;
        if (!nq) continue;  // (a batch nobody asks about is not uploaded)
        if (nq >= (1ull << 32)) return cx.fail(SAGE_HIP_ERR_UNSUPPORTED, "sage_hip_precursor_purity: 2^32 queries or more in one MS1 batch");
        unit_spec.clear();
        unit_qoff.clear();
        for (uint64_t sp = s0; sp < s1; ++sp)
            if (q_off[sp + 1] > q_off[sp]) {
                unit_spec.push_back((uint32_t)(sp - s0));
                unit_qoff.push_back((uint32_t)(q_off[sp] - first));
            }
        unit_qoff.push_back((uint32_t)nq);
        const uint32_t n_units = (uint32_t)unit_spec.size();
        qmz.resize(nq);
        qz.resize(nq);
        qlo.resize(nq);
        qhi.resize(nq);
        for (uint64_t i = 0; i < nq; ++i) {
            const uint64_t j = order[first + i];
            qmz[i] = in.precursor_mz[j];
            qz[i] = in.charge[j];
            qlo[i] = in.isolation_lo && in.isolation_hi ? in.isolation_lo[j] : nan;
            qhi[i] = in.isolation_lo && in.isolation_hi ? in.isolation_hi[j] : nan;
        }
        const uint64_t n = r.n_spectra, total = r.peak_off[n];
        HIP_TRY(d_off.reserve(n + 1));
        HIP_TRY(d_mz.reserve(total));
        HIP_TRY(d_in.reserve(total));
        HIP_TRY(d_spec.reserve(n_units));
        HIP_TRY(d_qoff.reserve((size_t)n_units + 1));
        HIP_TRY(d_sorted.reserve(n_units));
        HIP_TRY(d_qmz.reserve(nq));
        HIP_TRY(d_qz.reserve(nq));
        HIP_TRY(d_qlo.reserve(nq));
        HIP_TRY(d_qhi.reserve(nq));
        HIP_TRY(d_nw.reserve(nq));
        HIP_TRY(d_nm.reserve(nq));
        HIP_TRY(d_tot.reserve(nq));
        HIP_TRY(d_mat.reserve(nq));
        HIP_TRY(d_bel.reserve(nq));
        HIP_TRY(d_pur.reserve(nq));
        HIP_TRY(hipEventRecord(ev[0], cx.stream));
        HIP_TRY(hipMemcpyAsync(d_off.p, r.peak_off, (n + 1) * 8, hipMemcpyHostToDevice, cx.stream));
        if (total) {
            HIP_TRY(hipMemcpyAsync(d_mz.p, r.mz, total * 4, hipMemcpyHostToDevice, cx.stream));
            HIP_TRY(hipMemcpyAsync(d_in.p, r.intensities, total * 4, hipMemcpyHostToDevice, cx.stream));
        }
        HIP_TRY(hipMemcpyAsync(d_spec.p, unit_spec.data(), (size_t)n_units * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_qoff.p, unit_qoff.data(), ((size_t)n_units + 1) * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_qmz.p, qmz.data(), nq * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_qz.p, qz.data(), nq, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_qlo.p, qlo.data(), nq * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_qhi.p, qhi.data(), nq * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipEventRecord(ev[1], cx.stream));
        hipLaunchKernelGGL(sorted_flag_kernel, dim3((n_units + PUR_WAVES - 1) / PUR_WAVES), dim3(PUR_THREADS), 0, cx.stream, n_units, d_spec.p,
                           d_off.p, d_mz.p, d_sorted.p);
        HIP_TRY(hipGetLastError());
        const Queries dq{d_qmz.p, d_qz.p, d_qlo.p, d_qhi.p, d_nw.p, d_nm.p, d_tot.p, d_mat.p, d_bel.p, d_pur.p};
        hipLaunchKernelGGL(purity_kernel, dim3(n_units), dim3(PUR_THREADS), 0, cx.stream, d_spec.p, d_qoff.p, d_sorted.p, force_scan, d_off.p,
                           d_mz.p, d_in.p, dq, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[2], cx.stream));
        h_sorted.resize(n_units);
        h_nw.resize(nq);
        h_nm.resize(nq);
        h_tot.resize(nq);
        h_mat.resize(nq);
        h_bel.resize(nq);
        h_pur.resize(nq);
        HIP_TRY(hipMemcpyAsync(h_sorted.data(), d_sorted.p, n_units, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(h_nw.data(), d_nw.p, nq * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(h_nm.data(), d_nm.p, nq * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(h_tot.data(), d_tot.p, nq * 8, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(h_mat.data(), d_mat.p, nq * 8, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(h_bel.data(), d_bel.p, nq * 8, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(h_pur.data(), d_pur.p, nq * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipEventRecord(ev[3], cx.stream));
        HIP_TRY(hipStreamSynchronize(cx.stream));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        out.upload_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, ev[1], ev[2]));
        out.kernel_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[3]));
        out.device_ms += ms;
        for (uint32_t u = 0; u < n_units; ++u) ++(h_sorted[u] && !force_scan ? out.n_sorted_spectra : out.n_scanned_spectra);
        scatter(h_nw, order, first, out.n_window);
        scatter(h_nm, order, first, out.n_matched);
        scatter(h_tot, order, first, out.total);
        scatter(h_mat, order, first, out.matched);
        scatter(h_bel, order, first, out.below);
        scatter(h_pur, order, first, out.purity);
    }
    return true;
}

}  // namespace

int purity_on_device(int device, const SagePurityInput& in, SagePurityOutput& out, std::string& err) {
    Ctx cx;
    cx.prefix = "sage_hip_precursor_purity: ";
    if (purity_impl(cx, device, in, out)) return SAGE_HIP_OK;
    err = cx.err;
    return cx.code;
}

}  // namespace sagehip
