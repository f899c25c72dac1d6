// tmt.hip — isobaric reporter-ion extraction on the device: find_reporter_ions (sage tmt.rs:193-214), i.e.
// select_most_intense_peak(masses, intensities, label, tolerance, Some(-PROTON)) (spectrum.rs:134-159) for every label of every
// spectrum.  tmt_on_device (below) feeds it either the resident ProcessedSpectrum arrays of process_kernel (MS level 2) or
// the raw peaks as read (other levels: mass = mz - PROTON, computed here).
//
// Order-free selection.  Over peaks sorted stably by mass (total_cmp), the reference's scan keeps the LAST peak
// of the window whose intensity is >= the running maximum, starting from 0.0.  That is the last peak whose intensity equals
// M = max{intensity >= 0} of the window (float ==: 0.0 and -0.0 tie; NaN and negative values never win), i.e. the maximum of
// the key (intensity, total_cmp mass, position) over the window's peaks with intensity >= 0.  The key is a total order, so
// the maximum does not depend on the order the peaks are visited in: raw peaks need no sort, and every lane, wave and launch
// computes the same answer.  Position: in the processed spectrum (level 2, where it is sorted by mass, so the mass term never
// decides) or in the raw spectrum as given (other levels: the stable sort keeps equal masses in raw order).
//
// One wavefront per spectrum.  Lanes own labels (label = group * 64 + lane, any number of groups); per group the wave walks
// the spectrum 64 peaks at a time, keeps the peaks inside the reporter region [min lo, max hi] (ballot), and broadcasts each
// of them to every lane (v_readlane), which tests it against its own label's window.  No LDS, no atomics, any peak count.
#include <hip/hip_runtime.h>

#include <cmath>

#include "core.h"
#include "device_types.h"
#include "hip_host.h"

namespace sagehip {

namespace {

constexpr int TMT_WAVES = 4;  // wavefronts (spectra) per workgroup

__device__ __forceinline__ float bcast(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__global__ __launch_bounds__(64 * TMT_WAVES) void tmt_extract_kernel(uint32_t n, const uint64_t* __restrict__ off,
                                                                      const float* __restrict__ mass_or_mz,
                                                                      const float* __restrict__ inten, int subtract_proton,
                                                                      const float* __restrict__ lo, const float* __restrict__ hi,
                                                                      uint32_t n_labels, float region_lo, float region_hi,
                                                                      float* __restrict__ out_int, int32_t* __restrict__ out_idx) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t spec = (uint64_t)blockIdx.x * TMT_WAVES + (threadIdx.x >> 6);
    if (spec >= n) return;  // (wave-uniform: no workgroup barrier below)
    const uint64_t a = off[spec], e = off[spec + 1];
    for (uint32_t group = 0; group < n_labels; group += 64) {
        const uint32_t label = group + lane;
        const bool own = label < n_labels;
        const float llo = own ? lo[label] : NAN, lhi = own ? hi[label] : NAN;  // (NaN bounds: no peak is inside)
        bool found = false;
        uint32_t best_i = 0, best_pos = 0;  // intensity bits (-0.0 as 0.0), position in the spectrum
        int32_t best_m = 0;                 // total_cmp key of the mass
        for (uint64_t base = a; base < e; base += 64) {
            const uint64_t p = base + lane;
            float m = NAN, it = 0.0f;
            if (p < e) {
                m = mass_or_mz[p];
                if (subtract_proton) m = (m - sagecore::PROTON) * 1.0f;  // spectrum.rs:380-388
                it = inten[p];
            }
            // (a peak below 0 or NaN in intensity can never be selected; outside the region it is in no window)
            const bool keep = m >= region_lo && m <= region_hi && it >= 0.0f;
            uint64_t mask = __ballot(keep);
            while (mask) {
                const int src = __builtin_ctzll(mask);
                mask &= mask - 1;
                const float mj = bcast(m, src), ij = bcast(it, src);  // (read while the wave is converged)
                if (!(mj >= llo && mj <= lhi)) continue;
                const uint32_t ib = ij == 0.0f ? 0u : __float_as_uint(ij);
                const int32_t mk = sagecore::order_key(mj);
                const uint32_t pos = (uint32_t)(base - a) + (uint32_t)src;
                if (!found || ib > best_i || (ib == best_i && (mk > best_m || (mk == best_m && pos > best_pos)))) {
                    found = true;
                    best_i = ib;
                    best_m = mk;
                    best_pos = pos;
                }
            }
        }
        if (own) {
            const uint64_t o = spec * n_labels + label;
            out_int[o] = found ? inten[a + best_pos] : 0.0f;  // (the peak's own value: a selected -0.0 stays -0.0)
            if (out_idx) out_idx[o] = found ? (int32_t)best_pos : -1;
        }
    }
}

// reporter-ion extraction, one wavefront per spectrum (peaks [off[i], off[i+1]); subtract_proton: the array holds raw m/z); lo / hi:
// each label's window with the offset applied; region: [min lo, max hi].  out_*: [n * n_labels]
void launch_tmt_extract(uint32_t n, const uint64_t* off, const float* mass_or_mz, const float* inten, bool subtract_proton,
                        const float* lo, const float* hi, uint32_t n_labels, float region_lo, float region_hi, float* out_int,
                        int32_t* out_idx, void* stream) {
    if (!n || !n_labels) return;
    const uint32_t blocks = (n + TMT_WAVES - 1) / TMT_WAVES;
    hipLaunchKernelGGL(tmt_extract_kernel, dim3(blocks), dim3(64 * TMT_WAVES), 0, (hipStream_t)stream, n, off, mass_or_mz, inten,
                       subtract_proton ? 1 : 0, lo, hi, n_labels, region_lo, region_hi, out_int, out_idx);
}

// sage tmt.rs:314-352 quantify, minus the host-side row fields
bool tmt_impl(Ctx& cx, int device, const SageTmtInput& in, SageTmtOutput& out) {
    if ((in.n_batches && !in.batches) || (in.n_labels && !in.labels)) return cx.fail(SAGE_HIP_ERR_INVALID, "sage_hip_tmt: null array");
    if (in.tolerance.kind < 0 || in.tolerance.kind > 2) return cx.fail(SAGE_HIP_ERR_INVALID, "sage_hip_tmt: unknown tolerance kind");
    const bool ms2 = in.level == 2;
    const uint32_t L = in.n_labels;
    uint64_t n_total = 0;
    for (uint32_t b = 0; b < in.n_batches; ++b) {
        const SageRawBatch& r = in.batches[b];
        if (!r.n_spectra) continue;
        if (!r.peak_off || (ms2 && !r.precursor_charge)) return cx.fail(SAGE_HIP_ERR_INVALID, "sage_hip_tmt: null spectrum array");
        for (uint32_t i = 0; i < r.n_spectra; ++i) {
            if (r.peak_off[i + 1] < r.peak_off[i]) return cx.fail(SAGE_HIP_ERR_INVALID, "sage_hip_tmt: peak_off is not monotone");
            if (r.peak_off[i + 1] - r.peak_off[i] > (uint64_t)INT32_MAX)
                return cx.fail(SAGE_HIP_ERR_UNSUPPORTED, "sage_hip_tmt: a spectrum of more than 2^31 - 1 peaks (peak_index is i32)");
        }
        if (r.peak_off[r.n_spectra] && (!r.mz || !r.intensities)) return cx.fail(SAGE_HIP_ERR_INVALID, "sage_hip_tmt: missing peak arrays");
        n_total += r.n_spectra;
    }
    if (n_total && L && !out.intensity) return cx.fail(SAGE_HIP_ERR_INVALID, "sage_hip_tmt: null output array");
    out.upload_ms = out.process_ms = out.extract_ms = out.device_ms = 0.0f;
    if (!n_total || !L) return true;
    // each label's window in f32 on the host: Tolerance::bounds, then + offset (-PROTON); the region is their union's hull
    const sagecore::Tol tol{in.tolerance.kind, in.tolerance.lo, in.tolerance.hi};
    std::vector<float> lo(L), hi(L);
    float region_lo = INFINITY, region_hi = -INFINITY;
    for (uint32_t k = 0; k < L; ++k) {
        sagecore::offset_bounds(tol, in.labels[k], -sagecore::PROTON, lo[k], hi[k]);
        if (lo[k] < region_lo) region_lo = lo[k];
        if (hi[k] > region_hi) region_hi = hi[k];
    }
    HIP_TRY(hipSetDevice(device));
    Stream stream;  // (destroyed after the events)
    Events<4> ev;
    HIP_TRY(stream.create());
    HIP_TRY(ev.create());
    cx.stream = stream.s;
    DevBuf<float> dlo, dhi, dint;
    DevBuf<int32_t> didx;
    HIP_TRY(dlo.upload(lo.data(), L));
    HIP_TRY(dhi.upload(hi.data(), L));
    uint64_t row = 0;
    for (uint32_t b = 0; b < in.n_batches; ++b) {
        const SageRawBatch& r = in.batches[b];
        const uint32_t n = r.n_spectra;
        if (!n) continue;
        const uint64_t total = r.peak_off[n], cells = (uint64_t)n * L;
        HIP_TRY(dint.reserve(cells));
        if (out.peak_index) HIP_TRY(didx.reserve(cells));
        HIP_TRY(hipEventRecord(ev[0], cx.stream));
        ProcessScratch w;
        DevBuf<uint64_t> poff;
        DevBuf<float> pm, pi, tic;
        if (ms2) {  // the search's own preprocessing (min_peaks 0: every spectrum is quantified, runner.rs:334-359)
            std::vector<uint32_t> counts;
            std::vector<uint64_t> off;
            if (!process_raw_on_device(cx, &r, in.take_top_n, in.deisotope, in.min_deisotope_mz, 0, w, poff, pm, pi, tic, counts, off))
                return false;
        } else {    // mass = mz - PROTON in the kernel; the raw peaks as given
            HIP_TRY(poff.alloc((size_t)n + 1));
            HIP_TRY(pm.alloc(total));
            HIP_TRY(pi.alloc(total));
            HIP_TRY(hipMemcpyAsync(poff.p, r.peak_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, cx.stream));
            if (total) {
                HIP_TRY(hipMemcpyAsync(pm.p, r.mz, total * 4, hipMemcpyHostToDevice, cx.stream));
                HIP_TRY(hipMemcpyAsync(pi.p, r.intensities, total * 4, hipMemcpyHostToDevice, cx.stream));
            }
        }
        HIP_TRY(hipEventRecord(ev[1], cx.stream));
        launch_tmt_extract(n, poff.p, pm.p, pi.p, !ms2, dlo.p, dhi.p, L, region_lo, region_hi, dint.p, out.peak_index ? didx.p : nullptr,
                           cx.stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[2], cx.stream));
        HIP_TRY(hipMemcpyAsync(out.intensity + row * L, dint.p, cells * 4, hipMemcpyDeviceToHost, cx.stream));
        if (out.peak_index) HIP_TRY(hipMemcpyAsync(out.peak_index + row * L, didx.p, cells * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipEventRecord(ev[3], cx.stream));
        HIP_TRY(hipStreamSynchronize(cx.stream));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        (ms2 ? out.process_ms : out.upload_ms) += ms;
        HIP_TRY(hipEventElapsedTime(&ms, ev[1], ev[2]));
        out.extract_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[3]));
        out.device_ms += ms;
        row += n;
    }
    return true;
}

}  // namespace

int tmt_on_device(int device, const SageTmtInput& in, SageTmtOutput& out, std::string& err) {
    Ctx cx;
    if (tmt_impl(cx, device, in, out)) return SAGE_HIP_OK;
    err = cx.err;
    return cx.code;
}

}  // namespace sagehip
