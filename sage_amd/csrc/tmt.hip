// tmt.hip — isobaric reporter-ion extraction on the device: find_reporter_ions (sage tmt.rs:193-214), i.e.
// select_most_intense_peak(masses, intensities, label, tolerance, Some(-PROTON)) (spectrum.rs:134-159) for every label of every
// spectrum.  sage_hip_tmt (capi.hip) feeds it either the resident ProcessedSpectrum arrays of process_kernel (MS level 2) or
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

}  // namespace

void launch_tmt_extract(uint32_t n, const uint64_t* off, const float* mass_or_mz, const float* inten, bool subtract_proton,
                        const float* lo, const float* hi, uint32_t n_labels, float region_lo, float region_hi, float* out_int,
                        int32_t* out_idx, void* stream) {
    if (!n || !n_labels) return;
    const uint32_t blocks = (n + TMT_WAVES - 1) / TMT_WAVES;
    hipLaunchKernelGGL(tmt_extract_kernel, dim3(blocks), dim3(64 * TMT_WAVES), 0, (hipStream_t)stream, n, off, mass_or_mz, inten,
                       subtract_proton ? 1 : 0, lo, hi, n_labels, region_lo, region_hi, out_int, out_idx);
}

}  // namespace sagehip
