// lfq.hip — label-free MS1 quantification on the device: sage-core lfq.rs (build_feature_map, FeatureMap::quantify,
// Grid::add_entry / summarize_traces, Traces::integrate), isotopes.rs and fdr::picked_precursor (fdr.rs:228-287), for MS1
// spectra without ion mobility (sage_hip_lfq) and with a per-peak mobility column (sage_hip_lfq_im: lfq.rs:111-127, 267-286,
// 677-686, spectrum.rs:344-378).  The C entry points are in include/sage_hip.h.
//
// Stages, all on one stream:
//   feature map   host: the first confident target feature per peptide (confidence order), per-grid constants (rt_min,
//                 reference file, isotope distribution with libm expf); device: one thread per window writes the
//                 charge x isotope x forward/decoy windows (tol_bounds, no FMA), a radix sort on (rt total order << 32 |
//                 generation index) orders them by (rt, peptide, charge, isotope, decoy), a second, stable one on
//                 (page << 32 | mass_lo total order) sorts every 16 384-window page by mass_lo, ties in rt order.
//   MS1 peaks     mz - PROTON for every peak, a stable segmented radix sort per spectrum on the mass's total order.
//   traces        one thread per peak: its spectrum's aligned RT, the page range and the ±0.1 mass range with
//                 binary_search_slice's minus-one rule, the four exact predicates.  Count, scan, fill a contribution
//                 list in (spectrum, peak, match) order, a stable radix sort of the list on (grid slot, matrix row), then one
//                 thread per (grid, row) adds its contributions in list order — the additions of every cell in the order
//                 a sequential pass makes them, so every grid is bit-identical to it, without atomics.
//   integration   one block per grid: Gaussian smoothing (the Rust convolve loop), spectral angle, time warps (slack 75,
//                 `>=` keeps the last best offset), scores, best bin, peak bounds, Sum / Apex areas.  Only + * / sqrt on f64
//                 besides acos (the device's ocml acos); the RT factor powf(0.33) comes from a host table.
//   q-values      host: picked_precursor over the grids with a peak, a stable sort by f32 score in grid order.
// Ion mobility (only when a spectrum of the call has the column; otherwise none of it is allocated, launched or compiled into the
// kernels that run): one (mobility_lo, mobility_hi) record per selected feature, gathered per window through the same
// permutation as the mass bounds; the peaks' mobilities gathered through the MS1 sort's permutation; count / fill as the
// IM = true instances of the same templates, which read a window's record only after the four predicates of mass_lookup have
// passed, and test it only in spectra that have mobility.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "core.h"
#include "hip_host.h"

namespace sagehip {

namespace {

constexpr float RT_TOL = 0.0050f;      // lfq.rs:14
constexpr int K_WIDTH = 10;            // lfq.rs:16
constexpr int GRID = 100;              // lfq.rs:20
constexpr int N_ISO = 3;               // lfq.rs:22
constexpr uint32_t PAGE = 16 * 1024;   // lfq.rs:176
constexpr int SLACK = 75;              // lfq.rs:371
constexpr int IB = 256;                // threads of an integration block
constexpr int TB = 256;                // threads of a row-parallel block

SAGE_HD uint32_t total_key(float f) {  // ascending u32 order == f32::total_cmp
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t b = __float_as_uint(f);
#else
    uint32_t b;
    std::memcpy(&b, &f, 4);
#endif
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ inline float from_total_key(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// binary_search_slice (database.rs:549-561) over ascending total-order keys: (partition_point(< lo) - 1, saturating, then
// partition_point(<= hi) from there)
__device__ inline void search_keys(const uint32_t* keys, uint32_t n, uint32_t lo, uint32_t hi, uint32_t& left, uint32_t& right) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        if (keys[m] < lo) a = m + 1;
        else b = m;
    }
    left = a ? a - 1 : 0;
    a = left;
    b = n;
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        if (keys[m] <= hi) a = m + 1;
        else b = m;
    }
    right = a;
}

// ---- feature map ------------------------------------------------------------------------------------------------------
// generation index g = ((s * nz + zi) * 3 + isotope) * 2 + decoy over the selected features s (ascending peptide_idx)
__global__ void windows_kernel(uint32_t n_windows, uint32_t nz, uint32_t zmin, float ppm, const float* __restrict__ sel_rt,
                               const float* __restrict__ sel_mass, float* __restrict__ g_rt, float* __restrict__ g_lo,
                               float* __restrict__ g_hi, uint64_t* __restrict__ keys) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_windows) return;
    const uint32_t decoy = g & 1u, t = g >> 1;
    const uint32_t iso = t % N_ISO, zi = (t / N_ISO) % nz, s = t / N_ISO / nz;
    float mass = (sel_mass[s] + (float)iso * sagecore::NEUTRON) / (float)(zmin + zi);  // lfq.rs:147
    float rt = sel_rt[s];
    if (decoy) {
        mass = mass + 11.06f;                       // lfq.rs:163-165
        rt = fmaxf(rt - RT_TOL * 2.0f, 0.0f);       // lfq.rs:168
    }
    float lo, hi;
    sagecore::tol_bounds(sagecore::Tol{0, -ppm, ppm}, mass, lo, hi);
    g_rt[g] = rt;
    g_lo[g] = lo;
    g_hi[g] = hi;
    keys[g] = ((uint64_t)total_key(rt) << 32) | g;
}

// position j in rt order -> (page << 32 | mass_lo key), and the page's min_rt
__global__ void page_keys_kernel(uint32_t n_windows, const uint64_t* __restrict__ rt_sorted, const float* __restrict__ g_lo,
                                 uint64_t* __restrict__ keys, uint32_t* __restrict__ pos, uint32_t* __restrict__ min_rt_key) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_windows) return;
    const uint64_t k = rt_sorted[j];
    const uint32_t g = (uint32_t)k;
    keys[j] = ((uint64_t)(j / PAGE) << 32) | total_key(g_lo[g]);
    pos[j] = g;
    if (j % PAGE == 0) min_rt_key[j / PAGE] = (uint32_t)(k >> 32);  // the first of a page sorted by rt is its minimum
}

__global__ void gather_windows_kernel(uint32_t n_windows, const uint32_t* __restrict__ gen, const float* __restrict__ g_rt,
                                      const float* __restrict__ g_lo, const float* __restrict__ g_hi, float* __restrict__ w_rt,
                                      float* __restrict__ w_lo, float* __restrict__ w_hi, uint32_t* __restrict__ w_lo_key) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_windows) return;
    const uint32_t g = gen[j];
    w_rt[j] = g_rt[g];
    w_lo[j] = g_lo[g];
    w_hi[j] = g_hi[g];
    w_lo_key[j] = total_key(g_lo[g]);
}

// Tolerance::Pct(-pct, pct).bounds(feat.ims) of every selected feature (lfq.rs:111-115); x = mobility_lo, y = mobility_hi
__global__ void mobility_bounds_kernel(uint32_t n_sel, float pct, const float* __restrict__ sel_ims, float2* __restrict__ sel_mob) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_sel) return;
    float lo, hi;
    sagecore::tol_bounds(sagecore::Tol{1, -pct, pct}, sel_ims[s], lo, hi);
    sel_mob[s] = make_float2(lo, hi);
}

// every charge x isotope x forward/decoy window of a feature inherits its bounds (`..range`, `..fwd`: lfq.rs:145-164)
__global__ void gather_mobility_kernel(uint32_t n_windows, uint32_t per_feature, const uint32_t* __restrict__ gen,
                                       const float2* __restrict__ sel_mob, float2* __restrict__ w_mob) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_windows) return;
    w_mob[j] = sel_mob[gen[j] / per_feature];
}

// ---- MS1 peaks (spectrum.rs:380-412; with mobility :344-378) ------------------------------------------------------------------
__global__ void ms1_keys_kernel(uint64_t n, const float* __restrict__ mz, uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = total_key(mz[i] - sagecore::PROTON);  // (mass - PROTON) * 1.0
    idx[i] = (uint32_t)i;
}

__global__ void ms1_gather_kernel(uint64_t n, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                  const float* __restrict__ inten, float* __restrict__ mass, float* __restrict__ inten_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mass[i] = from_total_key(keys[i]);
    inten_out[i] = inten[idx[i]];
}

// the third column of spectrum.rs:346-362: the sort's permutation applied to the mobilities
__global__ void ms1_gather_mobility_kernel(uint64_t n, const uint32_t* __restrict__ idx, const float* __restrict__ mob,
                                           float* __restrict__ mob_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mob_out[i] = mob[idx[i]];
}

// ---- traces ---------------------------------------------------------------------------------------------------------------
struct SpecDev {
    float rt;            // aligned scan start time
    uint32_t page_lo, page_hi;
};

__global__ void spectrum_setup_kernel(uint32_t n_spec, const float* __restrict__ sst, const uint32_t* __restrict__ file_id,
                                      const SageAlignment* __restrict__ al, const uint32_t* __restrict__ min_rt_key,
                                      uint32_t n_pages, SpecDev* __restrict__ out) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_spec) return;
    const SageAlignment a = al[file_id[s]];
    const float rt = (sst[s] / a.max_rt) * a.slope + a.intercept;  // lfq.rs:240
    uint32_t lo, hi;
    search_keys(min_rt_key, n_pages, total_key(rt - RT_TOL), total_key(rt + RT_TOL), lo, hi);
    out[s] = SpecDev{rt, lo, hi};
}

struct WindowsDev {
    const float *rt, *lo, *hi;
    const uint32_t *lo_key, *gen;
    uint32_t n;
};

struct MobilityDev {  // read by the IM = true instances only
    const float2* window;      // [windows] (mobility_lo, mobility_hi), in the windows' final order
    const float* peak;         // [peaks] in sorted order
    const uint8_t* spectrum;   // [spectra] the spectrum has mobility
};

// Query::mass_lookup (lfq.rs:538-551) for one peak; f(window index) per match, in match order.  IM: mass_mobility_lookup
// (lfq.rs:677-686) when the peak's spectrum has mobility (`use_mob`), mass_lookup otherwise — the choice of lfq.rs:267.
template <bool IM, class F>
__device__ inline void lookup(const WindowsDev& w, const MobilityDev& md, const SpecDev& sp, float mass, bool use_mob, float mob,
                              F&& f) {
    const float min_rt = sp.rt - RT_TOL, max_rt = sp.rt + RT_TOL;
    const uint32_t klo = total_key(mass - 0.1f), khi = total_key(mass + 0.1f);
    for (uint32_t page = sp.page_lo; page < sp.page_hi; ++page) {
        const uint32_t a = page * PAGE;
        const uint32_t b = min(a + PAGE, w.n);
        uint32_t il, ir;
        search_keys(w.lo_key + a, b - a, klo, khi, il, ir);
        for (uint32_t e = a + il; e < a + ir; ++e) {
            const float rt = w.rt[e];
            if (rt <= max_rt && rt >= min_rt && mass >= w.lo[e] && mass <= w.hi[e]) {
                if constexpr (IM) {
                    if (use_mob) {
                        const float2 b = md.window[e];
                        if (!(b.y >= mob && b.x <= mob)) continue;
                    }
                }
                f(e);
            }
        }
    }
}

__device__ inline uint32_t spectrum_of(const uint64_t* peak_off, uint32_t n_spec, uint64_t i) {
    uint32_t a = 0, b = n_spec;  // last s with peak_off[s] <= i
    while (b - a > 1) {
        const uint32_t m = a + (b - a) / 2;
        if (peak_off[m] <= i) a = m;
        else b = m;
    }
    return a;
}

template <bool IM>
__global__ void count_kernel(uint64_t n_peaks, const uint64_t* __restrict__ peak_off, uint32_t n_spec,
                             const SpecDev* __restrict__ spec, const float* __restrict__ mass, WindowsDev w, MobilityDev md,
                             uint32_t* __restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_peaks) return;
    const uint32_t s = spectrum_of(peak_off, n_spec, i);
    const SpecDev sp = spec[s];
    bool use_mob = false;
    float mob = 0.0f;
    if constexpr (IM) {
        use_mob = md.spectrum[s] != 0;
        mob = md.peak[i];
    }
    uint32_t c = 0;
    lookup<IM>(w, md, sp, mass[i], use_mob, mob, [&](uint32_t) { ++c; });
    counts[i] = c;
}

struct SlotMap {  // window generation index -> grid slot (peptide, charge unless combined, decoy), matrix row
    uint32_t nz, combine, rows_per_slot;
    __device__ uint32_t slot(uint32_t g) const {
        const uint32_t decoy = g & 1u, t = g >> 1;
        const uint32_t sz = t / N_ISO;  // s * nz + zi
        return combine ? (sz / nz) * 2 + decoy : sz * 2 + decoy;
    }
};

template <bool IM>
__global__ void fill_kernel(uint64_t n_peaks, const uint64_t* __restrict__ peak_off, uint32_t n_spec,
                            const SpecDev* __restrict__ spec, const uint32_t* __restrict__ spec_file,
                            const float* __restrict__ mass, const float* __restrict__ inten, WindowsDev w, MobilityDev md, SlotMap sm,
                            const uint64_t* __restrict__ offsets, uint32_t* __restrict__ cell_key, uint32_t* __restrict__ cidx,
                            float* __restrict__ c_rt, float* __restrict__ c_int, uint8_t* __restrict__ slot_hit) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_peaks) return;
    const uint32_t s = spectrum_of(peak_off, n_spec, i);
    const SpecDev sp = spec[s];
    const uint32_t file = spec_file[s];
    const float it = inten[i];
    uint64_t c = offsets[i];
    bool use_mob = false;
    float mob = 0.0f;
    if constexpr (IM) {
        use_mob = md.spectrum[s] != 0;
        mob = md.peak[i];
    }
    lookup<IM>(w, md, sp, mass[i], use_mob, mob, [&](uint32_t e) {
        const uint32_t g = w.gen[e];
        const uint32_t slot = sm.slot(g);
        const uint32_t iso = (g >> 1) % N_ISO;
        cell_key[c] = slot * sm.rows_per_slot + file * N_ISO + iso;
        cidx[c] = (uint32_t)c;
        c_rt[c] = sp.rt;
        c_int[c] = it;
        slot_hit[slot] = 1;
        ++c;
    });
}

__global__ void grid_list_kernel(uint32_t n_slots, const uint8_t* __restrict__ hit, const uint32_t* __restrict__ grid_of_slot,
                                 uint32_t* __restrict__ slot_of_grid) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_slots && hit[s]) slot_of_grid[grid_of_slot[s]] = s;
}

// Grid::add_entry (lfq.rs:649-663) for every contribution of one matrix row, in list order
__global__ void row_reduce_kernel(uint64_t n_rows_total, uint32_t rows_per_slot, const uint32_t* __restrict__ slot_of_grid,
                                  const uint32_t* __restrict__ sorted_key, const uint32_t* __restrict__ sorted_idx, uint64_t n_contrib,
                                  const float* __restrict__ c_rt, const float* __restrict__ c_int, const float* __restrict__ slot_rt,
                                  double* __restrict__ matrix) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows_total) return;
    const uint32_t grid = (uint32_t)(t / rows_per_slot), row = (uint32_t)(t % rows_per_slot);
    const uint32_t slot = slot_of_grid[grid];
    const uint32_t key = slot * rows_per_slot + row;
    uint64_t a = 0, b = n_contrib;
    while (a < b) {
        const uint64_t m = a + (b - a) / 2;
        if (sorted_key[m] < key) a = m + 1;
        else b = m;
    }
    double* out = matrix + t * GRID;
    const float rt_min = slot_rt[slot] - RT_TOL;                // Grid::new, lfq.rs:638
    const float rt_step = (RT_TOL * 2.0f) / (float)GRID;       // lfq.rs:636
    for (uint64_t j = a; j < n_contrib && sorted_key[j] == key; ++j) {
        const uint32_t c = sorted_idx[j];
        const float srt = c_rt[c], intensity = c_int[c];
        const float f = floorf((srt - rt_min) / rt_step);
        // `as usize` saturates (negative and NaN -> 0), then .min(cols - 1)
        const uint32_t bin_lo = !(f > 0.0f) ? 0u : (f >= (float)(GRID - 1) ? (uint32_t)(GRID - 1) : (uint32_t)f);
        const uint32_t bin_hi = min(bin_lo + 1, (uint32_t)(GRID - 1));
        const float bin_lo_rt = (float)bin_lo * rt_step + rt_min;
        const float interp = (srt - bin_lo_rt) / rt_step;
        out[bin_lo] += (double)((1.0f - interp) * intensity);
        out[bin_hi] += (double)(interp * intensity);
    }
}

// ---- integration: one block per grid ---------------------------------------------------------------------------------------
struct IntegrateArgs {
    const double* matrix;       // [grids][files * 3][GRID]
    const uint32_t* slot_of_grid;
    const uint32_t* slot_file;  // reference file of a slot
    const float* slot_dist;     // [slots][3]
    const double* kernel;       // [K_WIDTH]
    const double* rt_factor;    // [GRID]
    double* dot;                // scratch [grids][files][GRID]
    double* angle;              // scratch [grids][files][GRID]
    uint32_t files;
    int32_t scoring, integration;
    double spectral_angle;
    // outputs [grids]
    uint8_t* has_peak;
    uint32_t *peak_rt, *left, *right;
    double *score, *sa;
    double* areas;              // [grids][files]
    int32_t* warps;             // [grids][files]
};

__global__ void __launch_bounds__(IB) integrate_kernel(IntegrateArgs A) {
    const uint32_t g = blockIdx.x;
    const uint32_t F = A.files;
    const uint32_t slot = A.slot_of_grid[g];
    const double* m = A.matrix + (size_t)g * F * N_ISO * GRID;
    double* dot = A.dot + (size_t)g * F * GRID;
    double* ang = A.angle + (size_t)g * F * GRID;
    int32_t* warps = A.warps + (size_t)g * F;
    __shared__ double s_dots[2 * SLACK + 1];
    __shared__ double s_spec[GRID], s_int[GRID], s_score[GRID];
    __shared__ double s_max;
    __shared__ int32_t s_best, s_left, s_right;
    const float d0 = A.slot_dist[slot * 3 + 0], d1 = A.slot_dist[slot * 3 + 1], d2 = A.slot_dist[slot * 3 + 2];
    const double ss_dist = (double)sqrtf(d0 * d0 + d1 * d1 + d2 * d2);  // lfq.rs:684-690
    const float dist[N_ISO] = {d0, d1, d2};

    // summarize_traces (lfq.rs:669-722): convolve (lfq.rs:612-627), spectral angle, dot product
    constexpr int MID = K_WIDTH - K_WIDTH / 2;
    for (uint32_t t = threadIdx.x; t < F * GRID; t += blockDim.x) {
        const uint32_t f = t / GRID;
        const int idx = (int)(t % GRID);
        const int ks = max(K_WIDTH - (MID + idx), 0), ws = max(idx - (MID - 1), 0);
        const int terms = min(K_WIDTH - ks, GRID - ws);
        double sa = 0.0, ss = 0.0;
        for (int iso = 0; iso < N_ISO; ++iso) {
            const double* row = m + ((size_t)f * N_ISO + iso) * GRID;
            double c = 0.0;
            for (int j = 0; j < terms; ++j) c = c + row[ws + j] * A.kernel[ks + j];
            sa += c * (double)dist[iso];
            ss += c * c;
        }
        const double sim = ss > 0.0 ? sa / (sqrt(ss) * ss_dist) : 0.0;
        ang[t] = 1.0 - 2.0 * acos(sim) / 3.141592653589793;  // std::f64::consts::PI
        dot[t] = sa;
    }
    __syncthreads();

    // find_time_warps (lfq.rs:386-411) against the reference file's dot product
    const double* ref = dot + (size_t)A.slot_file[slot] * GRID;
    for (uint32_t f = 0; f < F; ++f) {
        const double* run = dot + (size_t)f * GRID;
        for (int o = threadIdx.x; o <= 2 * SLACK; o += blockDim.x) {
            const int off = o - SLACK;
            double d = 0.0;
            for (int i = 0; i < GRID; ++i) {
                const int j = i + off;
                if (j >= 0 && j < GRID) d += ref[i] * run[j];
            }
            s_dots[o] = d;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int best_off = 0;
            double best = 0.0;
            for (int o = 0; o <= 2 * SLACK; ++o)
                if (s_dots[o] >= best) {
                    best_off = o - SLACK;
                    best = s_dots[o];
                }
            warps[f] = best_off;
        }
        __syncthreads();
    }

    // scores (lfq.rs:427-467) on the warped traces (apply_time_warps, lfq.rs:414-425: shifted[i] = run[i + warp] or 0.0)
    for (int col = threadIdx.x; col < GRID; col += blockDim.x) {
        double summed = 1.0, weighted = 0.0;
        for (uint32_t f = 0; f < F; ++f) {
            const int j = col + warps[f];
            const bool in = j >= 0 && j < GRID;
            const double sa = in ? ang[(size_t)f * GRID + j] : 0.0, dp = in ? dot[(size_t)f * GRID + j] : 0.0;
            weighted += sa * dp;
            summed += dp;
        }
        s_spec[col] = weighted / summed;
        s_int[col] = summed;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double mx = 0.0;
        for (int c = 0; c < GRID; ++c) mx = fmax(mx, s_int[c]);
        s_max = mx;
    }
    __syncthreads();
    for (int col = threadIdx.x; col < GRID; col += blockDim.x) {
        const double s = s_spec[col];
        double v;
        switch (A.scoring) {
            case SAGE_LFQ_RETENTION_TIME: v = A.rt_factor[col]; break;
            case SAGE_LFQ_SPECTRAL_ANGLE: v = s; break;
            case SAGE_LFQ_INTENSITY: v = sqrt(s_int[col] / s_max); break;
            default: v = s * (s * s) * A.rt_factor[col] * sqrt(s_int[col] / s_max); break;
        }
        s_score[col] = v;
    }
    __syncthreads();

    // integrate (lfq.rs:477-538): best bin, bounds
    if (threadIdx.x == 0) {
        int best_rt = 0;
        double best = 0.0;
        for (int rt = 0; rt < GRID; ++rt)
            if (s_score[rt] > best && s_spec[rt] >= A.spectral_angle) {
                best = s_score[rt];
                best_rt = rt;
            }
        A.has_peak[g] = best != 0.0;
        int left = best_rt > 0 ? best_rt - 1 : 0, right = best_rt + 1;
        if (best != 0.0) {
            const double threshold = best * 0.50;
            const int lmin = best_rt > GRID / 5 ? best_rt - GRID / 5 : 0;
            while (left > lmin && s_score[left] >= threshold && s_spec[left] >= A.spectral_angle) --left;
            const int rmax = min(GRID - 1, best_rt + 20);
            while (right < rmax && s_score[right] >= threshold && s_spec[right] >= A.spectral_angle) ++right;
        }
        A.peak_rt[g] = best_rt;
        A.left[g] = left;
        A.right[g] = right;
        A.score[g] = best;
        A.sa[g] = s_spec[best_rt];  // the same loop over files at best.rt (lfq.rs:523-532)
        s_best = best != 0.0 ? best_rt : -1;
        s_left = left;
        s_right = right;
    }
    __syncthreads();
    if (s_best < 0) return;
    for (uint32_t f = threadIdx.x; f < F; f += blockDim.x) {
        const int w = warps[f];
        const double* run = dot + (size_t)f * GRID;
        double area = 0.0;
        if (A.integration == SAGE_LFQ_SUM) {
            for (int j = s_left; j < s_right; ++j) {
                const int k = j + w;
                area += (k >= 0 && k < GRID) ? run[k] : 0.0;
            }
        } else {
            const int k = s_best + w;
            area = (k >= 0 && k < GRID) ? run[k] : 0.0;
        }
        A.areas[(size_t)g * F + f] = area;
    }
}

// ---- host helpers ------------------------------------------------------------------------------------------------------------
inline float powi_f32(float x, int k) { return k == 0 ? 1.0f : k == 1 ? x : k == 2 ? x * x : x * (x * x); }

// isotopes.rs:1-50 (f32; exp is libm expf, as f32::exp)
void conv4(const float* a, const float* b, float* o) {
    o[0] = a[0] * b[0];
    o[1] = a[0] * b[1] + a[1] * b[0];
    o[2] = a[0] * b[2] + a[1] * b[1] + a[2] * b[0];
    o[3] = a[0] * b[3] + a[1] * b[2] + a[2] * b[1] + a[3] * b[0];
}
void peptide_isotopes(uint32_t carbons, uint32_t sulfurs, float* out) {
    const float fact[4] = {1.0f, 1.0f, 2.0f, 6.0f};
    const float lam = (float)(uint16_t)carbons * 0.011f;
    float c13[4], s33[4], s35[4], s[4], c[4];
    for (int k = 0; k < 4; ++k) c13[k] = powi_f32(lam, k) * expf(-lam) / fact[k];
    const float l33 = (float)(uint16_t)sulfurs * 0.0076f, l35 = (float)(uint16_t)sulfurs * 0.044f;
    s35[0] = powi_f32(l35, 0) * expf(-l35);
    s35[1] = 0.0f;
    s35[2] = powi_f32(l35, 1) * expf(-l35);
    s35[3] = 0.0f;
    for (int k = 0; k < 4; ++k) s33[k] = powi_f32(l33, k) * expf(-l33) / fact[k];
    conv4(s33, s35, s);
    conv4(c13, s, c);
    const float mx = std::max(std::max(c[0], c[1]), c[2]);
    for (int k = 0; k < 3; ++k) out[k] = c[k] / mx;
}

// gaussian_kernel(0.5, 10), lfq.rs:592-608 (libm exp)
std::vector<double> gaussian_kernel(double sigma, int len) {
    const double step = 2.0 / (double)(len - 1);
    const double constant = 1.0 / (sigma * std::sqrt(2.0 * 3.141592653589793));
    std::vector<double> k(len);
    double sum = 0.0;
    for (int i = 0; i < len; ++i) {
        const double x = (double)i * step - 1.0;
        const double q = x / sigma;
        k[i] = constant * std::exp(-0.5 * (q * q));
    }
    for (int i = 0; i < len; ++i) sum += k[i];
    for (auto& v : k) v /= sum;
    return k;
}

inline uint32_t bits_for(uint64_t n) {  // radix-sort key width that holds 0..n-1
    uint32_t b = 1;
    while (b < 64 && (1ull << b) < n) ++b;
    return b;
}

inline uint32_t blocks(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

bool lfq_impl(Ctx& cx, const SageLfqInput& in, const SageLfqMobility* mobility, SageLfqOutput& out) {
    const SageLfqSettings& st = in.settings;
    // ion mobility takes part only if some spectrum of the call has the column (lfq.rs:267 decides per spectrum)
    bool im = false;
    for (uint32_t b = 0; mobility && !im && b < in.n_ms1; ++b) {
        if (!mobility[b].mobility) continue;
        for (uint32_t i = 0; !im && i < in.ms1[b].n_spectra; ++i) im = !mobility[b].has_mobility || mobility[b].has_mobility[i];
    }
    const uint32_t F = in.n_files;
    const uint32_t zmin = st.min_charge, nz = (uint32_t)st.max_charge - st.min_charge + 1;
    const bool combine = st.combine_charge_states != 0;
    const float ppm = std::fabs(st.ppm_tolerance);
    const double sa_thr = std::fabs(st.spectral_angle);
    Events<5> ev;
    HIP_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev[0], cx.stream));

    // -- feature map: selection (lfq.rs:99-141) on the host, features in confidence order
    std::vector<uint8_t> seen(in.n_peptides, 0);
    std::vector<uint32_t> pick;  // feature index per selected peptide
    std::vector<uint32_t> first(in.n_peptides, 0xFFFFFFFFu);
    for (uint64_t r = 0; r < in.n_features; ++r) {
        const uint64_t i = in.order ? in.order[r] : r;
        const SageFeature& f = in.features[i];
        if (!(in.peptide_q[i] <= st.peptide_q_value) || f.label != 1) continue;
        if (f.peptide_idx >= in.n_peptides || f.file_id >= F) {
            cx.code = SAGE_HIP_ERR_INVALID;
            cx.err = "sage_hip_lfq: a feature's peptide_idx or file_id is out of range";
            return false;
        }
        if (!seen[f.peptide_idx]) {
            seen[f.peptide_idx] = 1;
            first[f.peptide_idx] = (uint32_t)i;
        }
    }
    std::vector<uint32_t> sel_pep;
    std::vector<float> sel_rt, sel_mass, sel_ims;
    for (uint64_t p = 0; p < in.n_peptides; ++p)
        if (seen[p]) {
            const uint32_t i = first[p];
            sel_pep.push_back((uint32_t)p);
            sel_rt.push_back(in.aligned_rt[i]);
            sel_mass.push_back(in.features[i].calcmass);
            if (im) sel_ims.push_back(in.features[i].ims);
            pick.push_back(i);
        }
    const uint64_t S = sel_pep.size();
    const uint64_t W64 = S * nz * N_ISO * 2;
    const uint64_t per_pep = combine ? 2 : 2ull * nz;
    const uint64_t n_slots64 = S * per_pep;
    const uint64_t rows_per_slot = (uint64_t)F * N_ISO;
    if (W64 >= (1ull << 32) || n_slots64 * rows_per_slot >= (1ull << 32)) {
        cx.code = SAGE_HIP_ERR_UNSUPPORTED;
        cx.err = "sage_hip_lfq: more than 2^32 precursor windows or grid rows";
        return false;
    }
    const uint32_t W = (uint32_t)W64, n_slots = (uint32_t)n_slots64;
    // per grid slot: rt of its windows (Grid::new: rt_min = entry.rt - RT_TOL), reference file, isotope distribution
    std::vector<float> slot_rt(n_slots), slot_dist((size_t)n_slots * 3);
    std::vector<uint32_t> slot_file(n_slots);
    std::vector<uint32_t> slot_pep(n_slots);
    std::vector<uint8_t> slot_charge(n_slots), slot_decoy(n_slots);
    for (uint64_t s = 0; s < S; ++s) {
        float dist[3];
        const uint32_t p = sel_pep[s];
        peptide_isotopes(in.carbon[p], in.sulfur[p], dist);
        for (uint64_t k = 0; k < per_pep; ++k) {
            const uint64_t slot = s * per_pep + k;
            const bool decoy = k & 1;
            slot_rt[slot] = decoy ? std::fmax(sel_rt[s] - RT_TOL * 2.0f, 0.0f) : sel_rt[s];
            slot_file[slot] = in.features[pick[s]].file_id;
            slot_pep[slot] = p;
            slot_charge[slot] = combine ? 0 : (uint8_t)(zmin + k / 2);
            slot_decoy[slot] = decoy;
            std::memcpy(&slot_dist[slot * 3], dist, sizeof dist);
        }
    }
    const uint32_t n_pages = (W + PAGE - 1) / PAGE;
    DevBuf<float> d_sel_rt, d_sel_mass, g_rt, g_lo, g_hi, w_rt, w_lo, w_hi;
    DevBuf<uint64_t> k1, k1s, k2, k2s;
    DevBuf<uint32_t> pos, gen, w_lo_key, min_rt_key;
    HIP_TRY(d_sel_rt.alloc(S));
    HIP_TRY(d_sel_mass.alloc(S));
    for (auto* b : {&g_rt, &g_lo, &g_hi, &w_rt, &w_lo, &w_hi}) HIP_TRY(b->alloc(W));
    for (auto* b : {&k1, &k1s, &k2, &k2s}) HIP_TRY(b->alloc(W));
    for (auto* b : {&pos, &gen, &w_lo_key}) HIP_TRY(b->alloc(W));
    HIP_TRY(min_rt_key.alloc(n_pages));
    if (S) {
        HIP_TRY(hipMemcpyAsync(d_sel_rt.p, sel_rt.data(), S * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_sel_mass.p, sel_mass.data(), S * 4, hipMemcpyHostToDevice, cx.stream));
    }
    if (W) {
        windows_kernel<<<blocks(W, TB), TB, 0, cx.stream>>>(W, nz, zmin, ppm, d_sel_rt.p, d_sel_mass.p, g_rt.p, g_lo.p, g_hi.p, k1.p);
        HIP_TRY(with_scratch<DevBuf<uint8_t>>([&](void* t, size_t& b) {
                return rocprim::radix_sort_keys(t, b, k1.p, k1s.p, (size_t)W, 0, 64, cx.stream);
            }));
        page_keys_kernel<<<blocks(W, TB), TB, 0, cx.stream>>>(W, k1s.p, g_lo.p, k2.p, pos.p, min_rt_key.p);
        // stable: equal (page, mass_lo) keep their rt order
        HIP_TRY(with_scratch<DevBuf<uint8_t>>([&](void* t, size_t& b) {
                return rocprim::radix_sort_pairs(t, b, k2.p, k2s.p, pos.p, gen.p, (size_t)W, 0, 32 + bits_for(n_pages), cx.stream);
            }));
        gather_windows_kernel<<<blocks(W, TB), TB, 0, cx.stream>>>(W, gen.p, g_rt.p, g_lo.p, g_hi.p, w_rt.p, w_lo.p, w_hi.p,
                                                                   w_lo_key.p);
        HIP_TRY(hipGetLastError());
    }
    DevBuf<float> d_sel_ims;
    DevBuf<float2> d_sel_mob, w_mob;
    if (im && W) {
        HIP_TRY(d_sel_ims.alloc(S));
        HIP_TRY(d_sel_mob.alloc(S));
        HIP_TRY(w_mob.alloc(W));
        HIP_TRY(hipMemcpyAsync(d_sel_ims.p, sel_ims.data(), S * 4, hipMemcpyHostToDevice, cx.stream));
        mobility_bounds_kernel<<<blocks(S, TB), TB, 0, cx.stream>>>((uint32_t)S, st.mobility_pct_tolerance, d_sel_ims.p, d_sel_mob.p);
        gather_mobility_kernel<<<blocks(W, TB), TB, 0, cx.stream>>>(W, nz * N_ISO * 2, gen.p, d_sel_mob.p, w_mob.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[1], cx.stream));

    // -- MS1 spectra: concatenated in the order given
    uint64_t n_spec64 = 0, n_peaks = 0;
    for (uint32_t b = 0; b < in.n_ms1; ++b) {
        n_spec64 += in.ms1[b].n_spectra;
        if (in.ms1[b].n_spectra) n_peaks += in.ms1[b].peak_off[in.ms1[b].n_spectra] - in.ms1[b].peak_off[0];
    }
    if (n_spec64 >= (1ull << 31) || n_peaks >= (1ull << 32)) {
        cx.code = SAGE_HIP_ERR_UNSUPPORTED;
        cx.err = "sage_hip_lfq: more than 2^31 MS1 spectra or 2^32 MS1 peaks in one call";
        return false;
    }
    const uint32_t n_spec = (uint32_t)n_spec64;
    std::vector<uint64_t> h_off(n_spec + 1, 0);
    std::vector<float> h_mz(n_peaks), h_int(n_peaks), h_sst(n_spec);
    std::vector<uint32_t> h_file(n_spec);
    std::vector<uint8_t> h_has(im ? n_spec : 0, 0);  // per spectrum: it has mobility
    std::vector<uint64_t> batch_p0(in.n_ms1 + 1, 0);  // first peak of every batch in the concatenation
    {
        uint64_t s0 = 0, p0 = 0;
        for (uint32_t b = 0; b < in.n_ms1; ++b) {
            const SageRawBatch& r = in.ms1[b];
            for (uint32_t i = 0; i < r.n_spectra; ++i) {
                const uint64_t lo = r.peak_off[i], hi = r.peak_off[i + 1];
                if (hi < lo) {
                    cx.code = SAGE_HIP_ERR_INVALID;
                    cx.err = "sage_hip_lfq: MS1 peak_off not ascending";
                    return false;
                }
                std::memcpy(&h_mz[p0], r.mz + lo, (hi - lo) * 4);
                std::memcpy(&h_int[p0], r.intensities + lo, (hi - lo) * 4);
                if (im && mobility[b].mobility && (!mobility[b].has_mobility || mobility[b].has_mobility[i])) h_has[s0] = 1;
                p0 += hi - lo;
                h_off[s0 + 1] = p0;
                h_sst[s0] = r.scan_start_time ? r.scan_start_time[i] : 0.0f;
                h_file[s0] = r.file_id ? r.file_id[i] : 0;
                if (h_file[s0] >= F) {
                    cx.code = SAGE_HIP_ERR_INVALID;
                    cx.err = "sage_hip_lfq: an MS1 spectrum's file_id is >= n_files";
                    return false;
                }
                ++s0;
            }
            batch_p0[b + 1] = p0;
        }
    }
    DevBuf<uint64_t> d_off;
    DevBuf<float> d_mz, d_int_raw, d_mass, d_int, d_sst;
    DevBuf<uint32_t> d_file, mk, mks, mi, mis;
    DevBuf<SageAlignment> d_al;
    HIP_TRY(d_off.alloc(n_spec + 1));
    for (auto* b : {&d_mz, &d_int_raw, &d_mass, &d_int}) HIP_TRY(b->alloc(n_peaks));
    for (auto* b : {&mk, &mks, &mi, &mis}) HIP_TRY(b->alloc(n_peaks));
    HIP_TRY(d_sst.alloc(n_spec));
    HIP_TRY(d_file.alloc(n_spec));
    HIP_TRY(d_al.alloc(F));
    HIP_TRY(hipMemcpyAsync(d_off.p, h_off.data(), (n_spec + 1) * 8, hipMemcpyHostToDevice, cx.stream));
    if (n_peaks) {
        HIP_TRY(hipMemcpyAsync(d_mz.p, h_mz.data(), n_peaks * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_int_raw.p, h_int.data(), n_peaks * 4, hipMemcpyHostToDevice, cx.stream));
    }
    if (n_spec) {
        HIP_TRY(hipMemcpyAsync(d_sst.p, h_sst.data(), n_spec * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_file.p, h_file.data(), n_spec * 4, hipMemcpyHostToDevice, cx.stream));
    }
    if (F) HIP_TRY(hipMemcpyAsync(d_al.p, in.alignments, F * sizeof(SageAlignment), hipMemcpyHostToDevice, cx.stream));
    if (n_peaks) {
        ms1_keys_kernel<<<blocks(n_peaks, TB), TB, 0, cx.stream>>>(n_peaks, d_mz.p, mk.p, mi.p);
        HIP_TRY(with_scratch<DevBuf<uint8_t>>([&](void* t, size_t& b) {
                return rocprim::segmented_radix_sort_pairs(t, b, mk.p, mks.p, mi.p, mis.p, (unsigned int)n_peaks, n_spec,
                                                           d_off.p, d_off.p + 1, 0, 32, cx.stream);
            }));
        ms1_gather_kernel<<<blocks(n_peaks, TB), TB, 0, cx.stream>>>(n_peaks, mks.p, mis.p, d_int_raw.p, d_mass.p, d_int.p);
        HIP_TRY(hipGetLastError());
    }
    DevBuf<float> d_mob_raw, d_mob;
    DevBuf<uint8_t> d_spec_mob;
    if (im && n_peaks) {
        HIP_TRY(d_mob_raw.alloc(n_peaks));
        HIP_TRY(d_mob.alloc(n_peaks));
        HIP_TRY(d_spec_mob.alloc(n_spec));
        // The column of a batch goes up as it lies in the caller's array: peak_off ascends, so the peaks of a batch are one
        // range of it (no host copy of a third of the MS1 data).  The values inside spectra without mobility are never tested.
        for (uint32_t b = 0; b < in.n_ms1; ++b) {
            const uint64_t n = batch_p0[b + 1] - batch_p0[b];
            if (!n) continue;
            if (mobility[b].mobility)
                HIP_TRY(hipMemcpyAsync(d_mob_raw.p + batch_p0[b], mobility[b].mobility + in.ms1[b].peak_off[0], n * 4,
                                      hipMemcpyHostToDevice, cx.stream));
            else
                HIP_TRY(hipMemsetAsync(d_mob_raw.p + batch_p0[b], 0, n * 4, cx.stream));
        }
        HIP_TRY(hipMemcpyAsync(d_spec_mob.p, h_has.data(), n_spec, hipMemcpyHostToDevice, cx.stream));
        ms1_gather_mobility_kernel<<<blocks(n_peaks, TB), TB, 0, cx.stream>>>(n_peaks, mis.p, d_mob_raw.p, d_mob.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[2], cx.stream));

    // -- traces
    out.n_windows = W;
    out.n_grids = out.n_contributions = out.passing = 0;
    DevBuf<SpecDev> d_spec;
    DevBuf<uint32_t> counts;
    DevBuf<uint64_t> offs;
    HIP_TRY(d_spec.alloc(n_spec));
    HIP_TRY(counts.alloc(n_peaks));
    HIP_TRY(offs.alloc(n_peaks + 1));
    WindowsDev wd{w_rt.p, w_lo.p, w_hi.p, w_lo_key.p, gen.p, W};
    const MobilityDev md{w_mob.p, d_mob.p, d_spec_mob.p};
    uint64_t M = 0;
    if (n_peaks && W) {
        spectrum_setup_kernel<<<blocks(n_spec, TB), TB, 0, cx.stream>>>(n_spec, d_sst.p, d_file.p, d_al.p, min_rt_key.p, n_pages,
                                                                        d_spec.p);
        if (im) count_kernel<true><<<blocks(n_peaks, TB), TB, 0, cx.stream>>>(n_peaks, d_off.p, n_spec, d_spec.p, d_mass.p, wd, md, counts.p);
        else count_kernel<false><<<blocks(n_peaks, TB), TB, 0, cx.stream>>>(n_peaks, d_off.p, n_spec, d_spec.p, d_mass.p, wd, md, counts.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(with_scratch<DevBuf<uint8_t>>([&](void* t, size_t& b) {
                return rocprim::inclusive_scan(t, b, counts.p, offs.p + 1, (size_t)n_peaks, rocprim::plus<uint64_t>(), cx.stream);
            }));
        HIP_TRY(hipMemsetAsync(offs.p, 0, 8, cx.stream));
        HIP_TRY(hipMemcpyAsync(&M, offs.p + n_peaks, 8, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipStreamSynchronize(cx.stream));
    }
    out.n_contributions = M;
    if (M >= (1ull << 32)) {
        cx.code = SAGE_HIP_ERR_UNSUPPORTED;
        cx.err = "sage_hip_lfq: more than 2^32 (peak, window) matches in one call";
        return false;
    }
    DevBuf<uint32_t> ckey, ckeys, cidx, cidxs, grid_of_slot, slot_of_grid, d_slot_file;
    DevBuf<float> c_rt, c_int, d_slot_rt, d_slot_dist;
    DevBuf<uint8_t> slot_hit;
    for (auto* b : {&ckey, &ckeys, &cidx, &cidxs}) HIP_TRY(b->alloc(M));
    HIP_TRY(c_rt.alloc(M));
    HIP_TRY(c_int.alloc(M));
    HIP_TRY(slot_hit.alloc(n_slots));
    HIP_TRY(grid_of_slot.alloc(n_slots));
    HIP_TRY(hipMemsetAsync(slot_hit.p, 0, std::max<uint32_t>(n_slots, 1), cx.stream));
    uint32_t n_grids = 0;
    if (M) {
        SlotMap sm{nz, combine ? 1u : 0u, (uint32_t)rows_per_slot};
        if (im)
            fill_kernel<true><<<blocks(n_peaks, TB), TB, 0, cx.stream>>>(n_peaks, d_off.p, n_spec, d_spec.p, d_file.p, d_mass.p, d_int.p,
                                                                        wd, md, sm, offs.p, ckey.p, cidx.p, c_rt.p, c_int.p, slot_hit.p);
        else
            fill_kernel<false><<<blocks(n_peaks, TB), TB, 0, cx.stream>>>(n_peaks, d_off.p, n_spec, d_spec.p, d_file.p, d_mass.p, d_int.p,
                                                                         wd, md, sm, offs.p, ckey.p, cidx.p, c_rt.p, c_int.p, slot_hit.p);
        HIP_TRY(hipGetLastError());
        // stable: the contributions of one matrix row stay in (spectrum, peak, match) order
        HIP_TRY(with_scratch<DevBuf<uint8_t>>([&](void* t, size_t& b) {
                return rocprim::radix_sort_pairs(t, b, ckey.p, ckeys.p, cidx.p, cidxs.p, (size_t)M, 0,
                                                 bits_for(n_slots64 * rows_per_slot), cx.stream);
            }));
        HIP_TRY(with_scratch<DevBuf<uint8_t>>([&](void* t, size_t& b) {
                return rocprim::exclusive_scan(t, b, slot_hit.p, grid_of_slot.p, 0u, (size_t)n_slots, rocprim::plus<uint32_t>(),
                                               cx.stream);
            }));
        uint32_t last = 0;
        uint8_t last_hit = 0;
        HIP_TRY(hipMemcpyAsync(&last, grid_of_slot.p + n_slots - 1, 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(&last_hit, slot_hit.p + n_slots - 1, 1, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipStreamSynchronize(cx.stream));
        n_grids = last + last_hit;
    }
    out.n_grids = n_grids;
    if (n_grids > out.cap) {
        cx.code = SAGE_HIP_ERR_INVALID;
        cx.err = "sage_hip_lfq: output capacity " + std::to_string(out.cap) + " < " + std::to_string(n_grids) + " grids";
        return false;
    }
    const uint64_t rows_total = (uint64_t)n_grids * rows_per_slot;
    DevBuf<double> matrix, kern, rtf, dotb, angb, d_score, d_sa, d_areas;
    DevBuf<uint32_t> d_peak, d_left, d_right;
    DevBuf<int32_t> d_warps;
    DevBuf<uint8_t> d_has;
    HIP_TRY(slot_of_grid.alloc(n_grids));
    HIP_TRY(matrix.alloc(rows_total * GRID));
    HIP_TRY(d_slot_rt.alloc(n_slots));
    HIP_TRY(d_slot_file.alloc(n_slots));
    HIP_TRY(d_slot_dist.alloc((size_t)n_slots * 3));
    if (n_grids) {
        HIP_TRY(hipMemcpyAsync(d_slot_rt.p, slot_rt.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_slot_file.p, slot_file.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(d_slot_dist.p, slot_dist.data(), (size_t)n_slots * 12, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemsetAsync(matrix.p, 0, rows_total * GRID * 8, cx.stream));
        grid_list_kernel<<<blocks(n_slots, TB), TB, 0, cx.stream>>>(n_slots, slot_hit.p, grid_of_slot.p, slot_of_grid.p);
        row_reduce_kernel<<<blocks(rows_total, TB), TB, 0, cx.stream>>>(rows_total, (uint32_t)rows_per_slot, slot_of_grid.p, ckeys.p,
                                                                       cidxs.p, M, c_rt.p, c_int.p, d_slot_rt.p, matrix.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[3], cx.stream));

    // -- integration
    const std::vector<double> k = gaussian_kernel(0.5, K_WIDTH);
    std::vector<double> h_rtf(GRID);
    for (int rt = 0; rt < GRID; ++rt) {  // (1 - |rt - center| / center).powf(0.33), center = GRID / 2
        const int c = GRID / 2;
        h_rtf[rt] = std::pow(1.0 - ((double)std::abs(rt - c) / (double)c), 0.33);
    }
    HIP_TRY(kern.alloc(K_WIDTH));
    HIP_TRY(rtf.alloc(GRID));
    HIP_TRY(dotb.alloc((size_t)n_grids * F * GRID));
    HIP_TRY(angb.alloc((size_t)n_grids * F * GRID));
    HIP_TRY(d_score.alloc(n_grids));
    HIP_TRY(d_sa.alloc(n_grids));
    HIP_TRY(d_areas.alloc((size_t)n_grids * F));
    HIP_TRY(d_peak.alloc(n_grids));
    HIP_TRY(d_left.alloc(n_grids));
    HIP_TRY(d_right.alloc(n_grids));
    HIP_TRY(d_warps.alloc((size_t)n_grids * F));
    HIP_TRY(d_has.alloc(n_grids));
    std::vector<uint32_t> h_slot(n_grids);
    if (n_grids) {
        HIP_TRY(hipMemcpyAsync(kern.p, k.data(), K_WIDTH * 8, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemcpyAsync(rtf.p, h_rtf.data(), GRID * 8, hipMemcpyHostToDevice, cx.stream));
        HIP_TRY(hipMemsetAsync(d_areas.p, 0, (size_t)n_grids * F * 8, cx.stream));
        IntegrateArgs A{matrix.p, slot_of_grid.p, d_slot_file.p, d_slot_dist.p, kern.p, rtf.p, dotb.p, angb.p, F,
                        st.peak_scoring, st.integration, sa_thr, d_has.p, d_peak.p, d_left.p, d_right.p, d_score.p, d_sa.p,
                        d_areas.p, d_warps.p};
        integrate_kernel<<<n_grids, IB, 0, cx.stream>>>(A);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[4], cx.stream));
    if (n_grids) {
        HIP_TRY(hipMemcpyAsync(h_slot.data(), slot_of_grid.p, (size_t)n_grids * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(out.has_peak, d_has.p, n_grids, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(out.peak_rt, d_peak.p, (size_t)n_grids * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(out.left, d_left.p, (size_t)n_grids * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(out.right, d_right.p, (size_t)n_grids * 4, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(out.score, d_score.p, (size_t)n_grids * 8, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipMemcpyAsync(out.spectral_angle, d_sa.p, (size_t)n_grids * 8, hipMemcpyDeviceToHost, cx.stream));
        if (F) HIP_TRY(hipMemcpyAsync(out.areas, d_areas.p, (size_t)n_grids * F * 8, hipMemcpyDeviceToHost, cx.stream));
        if (out.warps && F)
            HIP_TRY(hipMemcpyAsync(out.warps, d_warps.p, (size_t)n_grids * F * 4, hipMemcpyDeviceToHost, cx.stream));
        if (out.matrix && rows_total)
            HIP_TRY(hipMemcpyAsync(out.matrix, matrix.p, rows_total * GRID * 8, hipMemcpyDeviceToHost, cx.stream));
    }
    HIP_TRY(hipStreamSynchronize(cx.stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    out.build_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[1], ev[2]));
    out.ms1_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[3]));
    out.trace_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[3], ev[4]));
    out.integrate_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[4]));
    out.device_ms = ms;

    // -- keys, then picked_precursor (fdr.rs:228-287) over the grids with a peak
    std::vector<uint32_t> with_peak;
    for (uint32_t g = 0; g < n_grids; ++g) {
        const uint32_t s = h_slot[g];
        out.peptide_idx[g] = slot_pep[s];
        out.charge[g] = slot_charge[s];
        out.decoy[g] = slot_decoy[s];
        out.q_value[g] = 1.0f;
        if (out.has_peak[g]) with_peak.push_back(g);
    }
    std::vector<uint32_t> keyed(with_peak.size());
    std::vector<uint32_t> sk(with_peak.size());
    for (size_t j = 0; j < with_peak.size(); ++j) sk[j] = total_key((float)out.score[with_peak[j]]);
    for (size_t j = 0; j < keyed.size(); ++j) keyed[j] = (uint32_t)j;
    std::stable_sort(keyed.begin(), keyed.end(), [&](uint32_t a, uint32_t b) { return sk[a] > sk[b]; });
    std::vector<float> q(keyed.size());
    float decoy = 1.0f, target = 0.0f;
    for (size_t j = 0; j < keyed.size(); ++j) {
        if (out.decoy[with_peak[keyed[j]]]) decoy += 1.0f;
        else target += 1.0f;
        q[j] = decoy / target;
    }
    float q_min = 1.0f;
    uint64_t passing = 0;
    for (size_t j = keyed.size(); j-- > 0;) {
        q_min = std::fmin(q_min, q[j]);
        const uint32_t g = with_peak[keyed[j]];
        out.q_value[g] = q_min;
        if (q_min <= 0.05f && !out.decoy[g]) ++passing;
    }
    out.passing = passing;
    return true;
}

}  // namespace

int lfq_on_device(int device, const SageLfqInput& in, const SageLfqMobility* mobility, SageLfqOutput& out, std::string& err) {
    return run_on_device(device, "sage_hip_lfq", "sage_hip_lfq: ", err, [&](Ctx& cx) { return lfq_impl(cx, in, mobility, out); });
}

}  // namespace sagehip
