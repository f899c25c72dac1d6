// rescore.hip — post-search rescoring on the device: the consumer of the Feature records.
//
//   score_psms            crates/sage/src/ml/linear_discriminant.rs:133-231
//   LDA::train / score    linear_discriminant.rs:57-133        (two streaming passes: class means, within-class scatter)
//   Gauss::solve          ml/gauss.rs:27-165                   (host: 20x20)
//   kde::Builder::build   ml/kde.rs:85-133, Estimator::posterior_error :143-168
//   spectrum_fdr          sage-cli/src/runner.rs:281-292, ml/qvalue.rs:8-36
//   picked_peptide/protein, Competition::assign_q_value        fdr.rs:60-187
//
// What runs where.  Everything that is O(n) or O(n x bins) is a kernel: the 20-column design (f64, never leaves HBM), the
// per-class sums and the 2 x 20 x 20 scatter accumulation, the projection, the kernel-density sums (bins x samples Gaussian
// evaluations — the only compute-heavy part), the descending sorts (rocprim radix sort on the f32 total order), the
// decoy/target prefix counts and the suffix minimum of the q-values, the per-key maxima of the picked competitions.  The
// host does the scalar glue between kernels: final addition of per-block partials, bandwidths, the Gauss-Jordan solve.
//
// Every long f64 reduction (class sums, within-class scatter, KDE means / deviations / Gaussian sums) is evaluated in the
// BLOCKED ORDER of detmath.h — consecutive blocks of DET_BLOCK elements, left to right inside a block (one sequential chain
// per (block, accumulator) on the device), block sums added left to right — and ln_1p / exp come from detmath.h's IEEE-only
// implementations.  That fixes every bit that reaches the Gauss-Jordan pivot search, so the fit-or-heuristic decision
// (gauss.rs:69-124 compares with `>=` / `== 0.0`; constant columns such as ims == 0 make some pivots candidates pure
// rounding noise) and everything downstream equal the CPU restatement of the same contract bit for bit; for n <= DET_BLOCK
// the order is the reference's own sequential one.  The one sum the reference keeps in f32 — `decoy += pep` of
// fdr.rs:93-101 — is evaluated strictly in order (seq_cumsum_kernel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/reverse_iterator.hpp>

#include "detmath.h"
#include "post_search.h"

namespace sagehip {

namespace {

constexpr int NF = 20;           // FEATURES, linear_discriminant.rs:19
constexpr uint32_t DB = sagedet::DET_BLOCK;  // elements per block of the blocked summation order

struct KdeDev {  // kde::Estimator on the device
    const double* bins;
    double min_score, score_step;
    uint32_t nbins;
};

// Estimator::posterior_error, kde.rs:146-168 (`as usize` saturates, NaN -> 0)
__device__ inline double kde_posterior_error(const KdeDev& e, double score) {
    const uint32_t last = e.nbins ? e.nbins - 1 : 0;
    const double r = floor((score - e.min_score) / e.score_step);
    const uint32_t lo = (!(r == r) || r <= 0.0) ? 0u : (r >= (double)last ? last : (uint32_t)r);
    const uint32_t hi = lo + 1 < last ? lo + 1 : last;
    const double lower = e.bins[lo], upper = e.bins[hi];
    const double lo_score = (double)lo * e.score_step + e.min_score;
    const double linear = (score - lo_score) / e.score_step;
    return lower + ((upper - lower) * linear);
}

__device__ inline uint32_t total_order_key(float f) {  // ascending u32 order == f32::total_cmp
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ inline float from_total_order_key(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// label -> decoy flag and the mass error of linear_discriminant.rs:140-144
__global__ __launch_bounds__(RB) void prep_kernel(const SageFeature* __restrict__ f, uint64_t n, int tol_kind,
                                                  uint8_t* __restrict__ decoy, double* __restrict__ dmass) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    decoy[i] = f[i].label == -1;
    dmass[i] = tol_kind == SAGE_TOL_PPM ? (double)f[i].delta_mass : (double)(f[i].expmass - f[i].calcmass);
}

// partial[b] = {min, max} over the block's slice (kde.rs:105-111; f64::min / max ignore a NaN operand, like fmin / fmax)
__global__ __launch_bounds__(RB) void minmax_kernel(const double* __restrict__ x, uint64_t n, double* __restrict__ partial) {
    __shared__ double lds[RB / 64];
    double mn = std::numeric_limits<double>::max(), mx = std::numeric_limits<double>::lowest();
    for (uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RB) {
        const double v = x[i];
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    }
    const double r0 = block_reduce(mn, OpMin(), lds), r1 = block_reduce(mx, OpMax(), lds);
    if (threadIdx.x == 0) {
        partial[blockIdx.x * 2] = r0;
        partial[blockIdx.x * 2 + 1] = r1;
    }
}

// Builder::build's `d` / `t` vectors (kde.rs:86-98): the scores split by class, each class in input order.
// dpos[i] = number of decoys before i (exclusive scan of the flags); xs[0, nd) = decoys, xs[nd, n) = targets.
__global__ __launch_bounds__(RB) void class_flags_kernel(const uint8_t* __restrict__ decoy, uint64_t n, uint32_t* __restrict__ flags) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i < n) flags[i] = decoy[i] ? 1u : 0u;
}
__global__ __launch_bounds__(RB) void class_split_kernel(const double* __restrict__ x, const uint8_t* __restrict__ decoy,
                                                         const uint32_t* __restrict__ dpos, uint64_t n, uint64_t nd,
                                                         double* __restrict__ xs) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    const uint64_t d = dpos[i];
    xs[decoy[i] ? d : nd + (i - d)] = x[i];
}

// part[b] = left-to-right sum over block b of x[i] (mode 0: ml/mod.rs:22-24) or (x[i] - mean)^2 (mode 1: ml/mod.rs:26-30).
// One thread = one block = one sequential chain (the blocked order of detmath.h).
__global__ __launch_bounds__(64) void blocked_sum_kernel(const double* __restrict__ x, uint64_t n, int mode, double mean,
                                                         double* __restrict__ part) {
    const uint64_t b = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t lo = b * DB, hi = lo + DB < n ? lo + DB : n;
    if (lo >= n) return;
    double s = 0.0;
    for (uint64_t i = lo; i < hi; ++i) {
        const double v = x[i];
        s += mode ? (v - mean) * (v - mean) : v;
    }
    part[b] = s;
}

// Kde::pdf numerators (kde.rs:34-50) of ONE class: partial[blk * nbins + bin] = sum over sample block blk, left to right, of
// exp(-0.5 ((score_bin - x_i) / h)^2).  One thread = one (bin, block) chain; the block's samples are staged in LDS once and
// read with wave-uniform addresses.
constexpr int KDE_THREADS = 256;
__global__ __launch_bounds__(KDE_THREADS) void kde_pdf_kernel(const double* __restrict__ xs, uint64_t n_c, double min_score,
                                                              double score_step, uint32_t nbins, double h,
                                                              double* __restrict__ partial) {
    __shared__ double tile[DB];
    const uint64_t lo = (uint64_t)blockIdx.y * DB;
    const uint32_t cnt = (uint32_t)(n_c - lo < DB ? n_c - lo : DB);
    for (uint32_t i = threadIdx.x; i < cnt; i += KDE_THREADS) tile[i] = xs[lo + i];
    __syncthreads();
    const uint32_t bin = blockIdx.x * KDE_THREADS + threadIdx.x;
    if (bin >= nbins) return;
    const double centre = ((double)bin * score_step) + min_score;
    double acc = 0.0;
    for (uint32_t i = 0; i < cnt; ++i) {
        const double u = (centre - tile[i]) / h;
        acc += sagedet::det_exp(-0.5 * (u * u));
    }
    partial[(uint64_t)blockIdx.y * nbins + bin] = acc;
}

// bins[b] = decoy_pdf * pi / (target_pdf * (1 - pi) + decoy_pdf * pi), then the monotone fold (kde.rs:113-126).  The block
// partials of a bin are added left to right from 0.0 (second level of the blocked order).  One workgroup.
__global__ __launch_bounds__(1024) void kde_finish_kernel(const double* __restrict__ part_d, uint32_t nblk_d,
                                                          const double* __restrict__ part_t, uint32_t nblk_t, uint32_t nbins,
                                                          double const_d, double const_t, double pi, int monotonic,
                                                          double* __restrict__ bins) {
    for (uint32_t b = threadIdx.x; b < nbins; b += blockDim.x) {
        double sd = 0.0, st = 0.0;
        for (uint32_t s = 0; s < nblk_d; ++s) sd += part_d[(uint64_t)s * nbins + b];
        for (uint32_t s = 0; s < nblk_t; ++s) st += part_t[(uint64_t)s * nbins + b];
        const double d = (sd / const_d) * pi;
        const double t = (st / const_t) * (1.0 - pi);
        bins[b] = d / (t + d);
    }
    __syncthreads();
    if (monotonic && threadIdx.x == 0) {
        double acc = bins[nbins - 1];
        for (uint32_t b = nbins; b-- > 0;) {
            acc = fmax(acc, bins[b]);
            bins[b] = acc;
        }
    }
}

// compute_features, linear_discriminant.rs:162-195: one 20-column f64 row per Feature
__global__ __launch_bounds__(RB) void rows_kernel(const SageFeature* __restrict__ f, uint64_t n, const double* __restrict__ dmass,
                                                  KdeDev mass_model, const float* __restrict__ aligned_rt,
                                                  const float* __restrict__ delta_rt, const float* __restrict__ delta_ims,
                                                  double* __restrict__ rows) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    const SageFeature p = f[i];
    double poisson = sagedet::det_log1p(-p.poisson);
    if (!isfinite(poisson)) poisson = 3.5;
    double* r = rows + i * NF;
    r[0] = (double)p.rank;
    r[1] = (double)p.charge;
    r[2] = sagedet::det_log1p(p.hyperscore);
    r[3] = sagedet::det_log1p(p.delta_next);
    r[4] = sagedet::det_log1p(p.delta_best);
    r[5] = kde_posterior_error(mass_model, dmass[i]);
    r[6] = (double)p.isotope_error;
    r[7] = (double)p.average_ppm;
    r[8] = poisson;
    r[9] = sagedet::det_log1p((double)p.matched_intensity_pct);
    r[10] = (double)p.matched_peaks;
    r[11] = sagedet::det_log1p((double)p.longest_b);
    r[12] = sagedet::det_log1p((double)p.longest_y);
    r[13] = (double)p.longest_y / (double)p.peptide_len;
    r[14] = sagedet::det_log1p((double)p.peptide_len);
    r[15] = (double)p.missed_cleavages;
    r[16] = (double)(aligned_rt ? aligned_rt[i] : p.rt);
    r[17] = (double)p.ims;
    const double drt = (double)(delta_rt ? delta_rt[i] : 0.999f), dims = (double)(delta_ims ? delta_ims[i] : 0.999f);
    r[18] = sqrt(drt < 0.001 ? 0.001 : (drt > 0.999 ? 0.999 : drt));  // f64::clamp: NaN stays NaN
    r[19] = sqrt(dims < 0.001 ? 0.001 : (dims > 0.999 ? 0.999 : dims));
}

// train's two passes over the rows (linear_discriminant.rs:70-82 class sums, :92-103 within-class scatter) in the REFERENCE'S
// ORDER: every accumulator is one running f64 sum over the rows of its class, strictly in row order — these sums decide,
// through the signed-maximum pivot search of the elimination (gauss.rs:97-108), whether the model is fitted at all, so a
// blocked order is not good enough.  One lane per accumulator, one workgroup (8 wavefronts) per CLASS: 20 chains
// for the class sums (SCATTER == false), 400 matrix entries for the scatter.  The workgroup walks ALL rows, 128 at a time: its
// 512 threads stage the tile's rows OF THEIR CLASS into LDS, compacted in row order (two ballots give the class mask; for the
// scatter the rows are centred on the way in, `row[j] - mu[j]` as the reference forms it), so the chain of a lane is two LDS
// reads, a multiply and THE add per row, nothing else; the next tile's loads are in flight meanwhile.  A wavefront that runs
// nearly alone retires an instruction every ~6 cycles, so instructions per row are what this costs: ~25 ms per million rows
// for both passes (a blocked order took 2 ms; a lane-per-accumulator walk with a class test per row 110 ms).
constexpr int SEQ_TILE = 128;                                     // rows per staged tile
constexpr int SEQ_THREADS = 512;
constexpr int SEQ_PER_THREAD = SEQ_TILE * NF / SEQ_THREADS;       // elements of a tile a thread moves (5)
static_assert(SEQ_TILE * NF % SEQ_THREADS == 0 && SEQ_TILE == 128, "two 64-row class masks per tile");
template <bool SCATTER>
__global__ __launch_bounds__(SEQ_THREADS) void seq_lda_kernel(const double* __restrict__ rows, const uint8_t* __restrict__ decoy,
                                                              uint64_t n, const double* __restrict__ class_mean /* [2][20], SCATTER only */,
                                                              double* __restrict__ out /* [2][20] resp. [2][400] */) {
    __shared__ double stage[2][SEQ_TILE][NF];
    __shared__ unsigned long long cmask[2][2];  // [buffer][rows 0..63 | 64..127]: bit r = the row belongs to this workgroup's class
    __shared__ double mu[NF];
    const uint32_t t = threadIdx.x;
    const uint32_t cls = blockIdx.y;  // 0 = decoys, 1 = targets (linear_discriminant.rs:73)
    const bool owner = SCATTER ? t < NF * NF : t < NF;
    const uint32_t ej = owner ? (SCATTER ? t / NF : t) : 0, ek = owner && SCATTER ? t % NF : 0;
    if (SCATTER && t < NF) mu[t] = class_mean[cls * NF + t];
    __syncthreads();
    double reg[SEQ_PER_THREAD];
    bool reg_mine = false;
    auto load_tile = [&](uint64_t base) {  // element e = t + 512 i of the tile: row e / 20, column e % 20; thread t < 128: row t's class
        const uint64_t cnt = n - base < SEQ_TILE ? n - base : SEQ_TILE;
#pragma unroll
        for (int i = 0; i < SEQ_PER_THREAD; ++i) {
            const uint32_t e = t + (uint32_t)SEQ_THREADS * (uint32_t)i;
            reg[i] = e < cnt * NF ? rows[base * NF + e] : 0.0;
        }
        reg_mine = t < cnt && (decoy[base + t] ? 0u : 1u) == cls;
    };
    auto store_tile = [&](int buf) {  // (every thread calls it: there is a barrier inside)
        if (t < SEQ_TILE) {
            const unsigned long long m = __ballot(reg_mine);
            if ((t & 63u) == 0) cmask[buf][t >> 6] = m;
        }
        __syncthreads();
        const unsigned long long m0 = cmask[buf][0], m1 = cmask[buf][1];
#pragma unroll
        for (int i = 0; i < SEQ_PER_THREAD; ++i) {
            const uint32_t e = t + (uint32_t)SEQ_THREADS * (uint32_t)i, r = e / NF, c = e % NF;
            const unsigned long long half = r < 64 ? m0 : m1, bit = 1ull << (r & 63u);
            if (half & bit) {  // the row's place among the tile's rows of this class, in row order
                const uint32_t rank = (r < 64 ? 0u : (uint32_t)__popcll(m0)) + (uint32_t)__popcll(half & (bit - 1ull));
                stage[buf][rank][c] = SCATTER ? reg[i] - mu[c] : reg[i];
            }
        }
    };
    double acc = 0.0;
    if (n) load_tile(0);
    store_tile(0);
    __syncthreads();
    int buf = 0;
    for (uint64_t base = 0; base < n; base += SEQ_TILE, buf ^= 1) {
        const bool more = base + SEQ_TILE < n;
        if (more) load_tile(base + SEQ_TILE);
        if (owner) {
            const uint32_t cnt = (uint32_t)(__popcll(cmask[buf][0]) + __popcll(cmask[buf][1]));
            const double* pj = &stage[buf][0][ej];
            const double* pk = &stage[buf][0][ek];
#pragma unroll 4
            for (uint32_t r = 0; r < cnt; ++r) acc += SCATTER ? pj[r * NF] * pk[r * NF] : pj[r * NF];  // in row order
        }
        if (more) store_tile(buf ^ 1);
        __syncthreads();
    }
    if (owner) out[(size_t)cls * (SCATTER ? NF * NF : NF) + t] = acc;
}

struct Coef {
    double w[NF];
};

// lda.score (:130-133): left-to-right sum from 0.0, identical to the reference given identical rows and coefficients
__global__ __launch_bounds__(RB) void project_kernel(const double* __restrict__ rows, uint64_t n, Coef coef,
                                                     double* __restrict__ disc) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NF; ++j) s += coef.w[j] * rows[i * NF + j];
    disc[i] = s;
}

// :219-229
__global__ __launch_bounds__(RB) void pep_kernel(const double* __restrict__ disc, uint64_t n, KdeDev kde,
                                                 float* __restrict__ discriminant, float* __restrict__ posterior_error) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    discriminant[i] = (float)disc[i];
    float pe = (float)log10(kde_posterior_error(kde, disc[i]));
    if (isinf(pe)) pe = -324.0f;
    posterior_error[i] = pe;
}

// runner.rs:285-288 heuristic when the model cannot be fitted; posterior_error keeps the Feature default 1.0
__global__ __launch_bounds__(RB) void heuristic_kernel(const SageFeature* __restrict__ f, uint64_t n,
                                                       float* __restrict__ discriminant, float* __restrict__ posterior_error) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    discriminant[i] = sagedet::det_log1pf((float)(-f[i].poisson)) + f[i].longest_y_pct / 3.0f;
    posterior_error[i] = 1.0f;
}

__global__ __launch_bounds__(RB) void sort_keys_kernel(const float* __restrict__ score, uint32_t n, uint32_t* __restrict__ keys,
                                                       uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    keys[i] = total_order_key(score[i]);
    idx[i] = i;
}

// flags[j] = 1 when the j-th best PSM is a decoy (input of the prefix count of qvalue.rs:16-24)
__global__ __launch_bounds__(RB) void decoy_flags_kernel(const uint32_t* __restrict__ order, const uint8_t* __restrict__ decoy,
                                                         uint32_t n, uint32_t* __restrict__ flags) {
    const uint32_t j = blockIdx.x * RB + threadIdx.x;
    if (j < n) flags[j] = decoy[order[j]] ? 1u : 0u;
}

// qvalue.rs:16-24 on the sorted order: q[j] = (1 + decoys in [0, j]) / (targets in [0, j]), already folded with the 1.0 the
// reverse cumulative minimum starts from (min is associative: min(1, min(a, b)) == min(min(1, a), min(1, b)))
__global__ __launch_bounds__(RB) void q_from_counts_kernel(const uint32_t* __restrict__ decoy_cum, uint32_t n, float* __restrict__ q) {
    const uint32_t j = blockIdx.x * RB + threadIdx.x;
    if (j >= n) return;
    const uint32_t d = 1u + decoy_cum[j], t = (j + 1u) - decoy_cum[j];  // `let mut decoy = 1; let mut target = 0;`
    q[j] = fminf(1.0f, (float)d / (float)t);
}

struct OpFmin {
    __device__ float operator()(float a, float b) const { return fminf(a, b); }
};

// rows passing `threshold` after the reverse cumulative minimum (qvalue.rs:31-33; fdr.rs:108-110 also requires a target row)
__global__ __launch_bounds__(RB) void count_passing_kernel(const float* __restrict__ q, uint32_t n, const uint8_t* __restrict__ row_decoy,
                                                           float threshold, unsigned long long* __restrict__ passing) {
    const uint32_t j = blockIdx.x * RB + threadIdx.x;
    const bool pass = j < n && q[j] <= threshold && !(row_decoy && row_decoy[j]);
    const unsigned long long b = __ballot(pass);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(passing, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(RB) void scatter_by_order_kernel(const uint32_t* __restrict__ order, const float* __restrict__ q,
                                                              uint32_t n, float* __restrict__ out) {
    const uint32_t j = blockIdx.x * RB + threadIdx.x;
    if (j < n) out[order[j]] = q[j];
}

// ---- picked competitions (fdr.rs) --------------------------------------------------------------------------------------
// side[2 * key + s] (s = 0 forward, 1 reverse) holds the total-order key of the best discriminant of that side, 0 = absent
// (0 is the key of a negative NaN with full payload; every real score maps above it).
__global__ __launch_bounds__(RB) void picked_max_kernel(const uint32_t* __restrict__ key, const uint8_t* __restrict__ decoy,
                                                        const float* __restrict__ score, uint64_t n, uint32_t* __restrict__ side) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n || key[i] == 0xFFFFFFFFu) return;
    float s = score[i];
    if (!(s == s)) s = -std::numeric_limits<float>::max();  // f32::max(f32::MIN, NaN) == f32::MIN (fdr.rs:137,141)
    s = fmaxf(s, -std::numeric_limits<float>::max());
    atomicMax(&side[2ull * key[i] + (decoy[i] ? 1 : 0)], total_order_key(s));
}

// per key: the winner of the competition for the KDE fit (Competition::score / is_decoy, fdr.rs:42-49) and the sort keys of
// its rows in (key, forward-before-reverse) order
__global__ __launch_bounds__(RB) void picked_rows_kernel(const uint32_t* __restrict__ side, uint32_t n_keys,
                                                         double* __restrict__ winner, uint8_t* __restrict__ winner_decoy,
                                                         uint32_t* __restrict__ row_key, uint32_t* __restrict__ row_id,
                                                         uint32_t* __restrict__ counters /* [0] rows present, [1] unused keys */) {
    const uint32_t g = blockIdx.x * RB + threadIdx.x;
    if (g >= n_keys) return;
    const uint32_t kf = side[2 * g], kr = side[2 * g + 1];
    const float FMIN = -std::numeric_limits<float>::max();
    const float fwd = kf ? from_total_order_key(kf) : FMIN, rev = kr ? from_total_order_key(kr) : FMIN;
    winner[g] = (double)fmaxf(fwd, rev);
    winner_decoy[g] = rev >= fwd;
    row_key[2 * g] = kf;
    row_key[2 * g + 1] = kr;
    row_id[2 * g] = 2 * g;
    row_id[2 * g + 1] = 2 * g + 1;
    const uint32_t present = (kf != 0) + (kr != 0);
    if (present) atomicAdd(&counters[0], present);
    else atomicAdd(&counters[1], 1u);
}

// rows in sorted order: their posterior error (fdr.rs:94), side, and the target flag the prefix count runs over; pep is
// zero-padded to a whole number of seq_cumsum_kernel tiles
__global__ __launch_bounds__(RB) void picked_pep_kernel(const uint32_t* __restrict__ sorted_key, const uint32_t* __restrict__ sorted_id,
                                                        uint32_t m, uint32_t m_padded, KdeDev est, float* __restrict__ pep,
                                                        uint8_t* __restrict__ row_decoy, uint32_t* __restrict__ target_flag) {
    const uint32_t j = blockIdx.x * RB + threadIdx.x;
    if (j >= m_padded) return;
    if (j >= m) {
        pep[j] = 0.0f;
        return;
    }
    pep[j] = (float)kde_posterior_error(est, (double)from_total_order_key(sorted_key[j]));
    const uint32_t dec = sorted_id[j] & 1;
    row_decoy[j] = (uint8_t)dec;
    target_flag[j] = dec ^ 1u;
}

// fdr.rs:91-101: decoy = 1.0; target = 0.0; for row { decoy += pep; if !row.decoy { target += 1.0 }; q = decoy / target }.
// `decoy` is an f32 running sum whose rounding depends on the order, so it is evaluated strictly in row order by ONE
// wavefront whose lanes all carry the same running sum: one dependent v_add_f32 per row.  The wavefront streams the pep
// values through LDS in tiles of 1024 rows (the next tile's global loads are in flight while the current one is summed),
// reads them back with uniform addresses, parks the running sums of 64 rows in LDS and lane k stores the sum as it stood
// after row k.  Nothing in the loop waits on global memory.  `target` counts whole numbers (exact in f32 below 2^24) and
// comes from the parallel prefix count; the division is picked_q_kernel's.
constexpr int CS_TILE = 1024;
__global__ __launch_bounds__(64) void seq_cumsum_kernel(const float* __restrict__ pep /* zero-padded to m_padded */,
                                                        uint32_t m_padded /* multiple of CS_TILE, > 0 */,
                                                        float* __restrict__ dsum) {
    __shared__ float4 tile[CS_TILE / 4];
    __shared__ float4 run[16];
    const uint32_t lane = threadIdx.x;
    const float4* src = reinterpret_cast<const float4*>(pep);
    float4 n0 = src[lane], n1 = src[64 + lane], n2 = src[128 + lane], n3 = src[192 + lane];
    float d = 1.0f;
    for (uint32_t base = 0; base < m_padded; base += CS_TILE) {
        tile[lane] = n0;
        tile[64 + lane] = n1;
        tile[128 + lane] = n2;
        tile[192 + lane] = n3;
        __syncthreads();
        {  // next tile (the last iteration re-reads its own tile: no branch, nothing spilled)
            const uint32_t nb = (base + CS_TILE < m_padded ? base + CS_TILE : base) / 4;
            n0 = src[nb + lane];
            n1 = src[nb + 64 + lane];
            n2 = src[nb + 128 + lane];
            n3 = src[nb + 192 + lane];
        }
        float4 cur[16], nxt[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) cur[i] = tile[i];  // uniform addresses: every lane reads the same 64 values
        for (int c = 0; c < CS_TILE / 64; ++c) {
            const int cn = c + 1 < CS_TILE / 64 ? c + 1 : c;
#pragma unroll
            for (int i = 0; i < 16; ++i) nxt[i] = tile[cn * 16 + i];  // in flight during the 64 dependent adds below
            float4 r[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                d = d + cur[i].x;
                r[i].x = d;
                d = d + cur[i].y;
                r[i].y = d;
                d = d + cur[i].z;
                r[i].z = d;
                d = d + cur[i].w;
                r[i].w = d;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) run[i] = r[i];
            __syncthreads();
            dsum[base + c * 64 + lane] = reinterpret_cast<const float*>(run)[lane];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 16; ++i) cur[i] = nxt[i];
        }
    }
}

// q = decoy / target, folded with the 1.0 the reverse minimum starts from (a NaN q — no target yet and a NaN posterior
// error — becomes 1.0, as f32::min makes it in fdr.rs:107)
__global__ __launch_bounds__(RB) void picked_q_kernel(const float* __restrict__ dsum, const uint32_t* __restrict__ target_cum,
                                                      uint32_t m, float* __restrict__ q) {
    const uint32_t j = blockIdx.x * RB + threadIdx.x;
    if (j < m) q[j] = fminf(1.0f, dsum[j] / (float)target_cum[j]);
}

__global__ __launch_bounds__(RB) void picked_scatter_kernel(const uint32_t* __restrict__ sorted_id, const float* __restrict__ q,
                                                            uint32_t m, float* __restrict__ side_q) {
    const uint32_t j = blockIdx.x * RB + threadIdx.x;
    if (j < m) side_q[sorted_id[j]] = q[j];
}

__global__ __launch_bounds__(RB) void picked_gather_kernel(const uint32_t* __restrict__ key, const uint8_t* __restrict__ decoy,
                                                           uint64_t n, const float* __restrict__ side_q, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    out[i] = key[i] == 0xFFFFFFFFu ? 1.0f : side_q[2ull * key[i] + (decoy[i] ? 1 : 0)];
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// the pool and the stream of the call in scope on this thread (ScratchScope, below)
thread_local hipStream_t tl_stream = nullptr;
thread_local bool tl_pooled = false;

struct KdeFit {
    Buf<double> bins;
    KdeDev dev{};
};

// left-to-right fold of block partials from +0.0 (second level of the blocked order)
double fold_partials(const std::vector<double>& part) {
    double s = 0.0;
    for (double v : part) s += v;
    return s;
}

// blocked-order sum of x[0, n) (mode 0) or of (x - mean)^2 (mode 1): chains on the device, block partials folded on the host
bool blocked_sum(Ctx& cx, const double* d_x, uint64_t n, int mode, double mean, double& out) {
    out = 0.0;
    if (n == 0) return true;
    const uint64_t nblk = (n + DB - 1) / DB;
    Buf<double> part;
    HIP_TRY(part.alloc(nblk));
    blocked_sum_kernel<<<grid_for(nblk, 64), 64, 0, cx.stream>>>(d_x, n, mode, mean, part.p);
    std::vector<double> h(nblk);
    HIP_TRY(hipMemcpyAsync(h.data(), part.p, nblk * 8, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipStreamSynchronize(cx.stream));
    out = fold_partials(h);
    return true;
}

// kde::Builder{monotonic, bins, bw_adjust = x * bw_mult}.build(scores, decoys)  (kde.rs:85-133)
bool kde_build(Ctx& cx, const double* d_scores, const uint8_t* d_decoy, uint64_t n, bool monotonic, uint32_t nbins,
               double bw_mult, KdeFit& fit) {
    // the class vectors `d` and `t` (kde.rs:86-98), each in input order
    Buf<uint32_t> flags, dpos;
    Buf<double> xs, mm;
    HIP_TRY(flags.alloc(n));
    HIP_TRY(dpos.alloc(n));
    HIP_TRY(xs.alloc(n));
    class_flags_kernel<<<grid_for(n, RB), RB, 0, cx.stream>>>(d_decoy, n, flags.p);
    if (!exclusive_count(cx, flags.p, dpos.p, n)) return false;
    uint32_t last_pos = 0, last_flag = 0;
    HIP_TRY(hipMemcpyAsync(&last_pos, dpos.p + (n - 1), 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(&last_flag, flags.p + (n - 1), 4, hipMemcpyDeviceToHost, cx.stream));
    const uint32_t nb = blocks_for(n);
    HIP_TRY(mm.alloc((size_t)nb * 2));
    minmax_kernel<<<nb, RB, 0, cx.stream>>>(d_scores, n, mm.p);
    std::vector<double> hmm((size_t)nb * 2);
    HIP_TRY(hipMemcpyAsync(hmm.data(), mm.p, hmm.size() * 8, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipStreamSynchronize(cx.stream));
    const uint64_t cnt_u[2] = {(uint64_t)last_pos + last_flag, n - ((uint64_t)last_pos + last_flag)};
    class_split_kernel<<<grid_for(n, RB), RB, 0, cx.stream>>>(d_scores, d_decoy, dpos.p, n, cnt_u[0], xs.p);
    double mn = std::numeric_limits<double>::max(), mx = std::numeric_limits<double>::lowest();
    for (uint32_t b = 0; b < nb; ++b) {
        mn = std::fmin(mn, hmm[b * 2]);
        mx = std::fmax(mx, hmm[b * 2 + 1]);
    }
    const double* cls_x[2] = {xs.p, xs.p + cnt_u[0]};
    // Kde::new (kde.rs:21-32) over mean / std of ml/mod.rs:22-30
    double bw[2], constant[2];
    for (int c = 0; c < 2; ++c) {
        const double cnt = (double)cnt_u[c];
        double sum = 0.0, ss = 0.0;
        if (!blocked_sum(cx, cls_x[c], cnt_u[c], 0, 0.0, sum)) return false;
        const double mean = sum / cnt;
        if (!blocked_sum(cx, cls_x[c], cnt_u[c], 1, mean, ss)) return false;
        const double sigma = std::sqrt(ss / cnt);
        bw[c] = (sigma * std::pow((4.0 / 3.0) / cnt, 1.0 / 5.0)) * bw_mult;
        constant[c] = std::sqrt(2.0 * M_PI) * bw[c] * cnt;
    }
    const double pi = (double)cnt_u[0] / (double)n;
    const double step = (mx - mn) / (double)(nbins - 1);
    const uint32_t nblk[2] = {(uint32_t)((cnt_u[0] + DB - 1) / DB), (uint32_t)((cnt_u[1] + DB - 1) / DB)};
    Buf<double> pdf_partial[2];
    HIP_TRY(fit.bins.alloc(nbins));
    for (int c = 0; c < 2; ++c) {
        HIP_TRY(pdf_partial[c].alloc((size_t)nblk[c] * nbins));
        if (nblk[c])
            kde_pdf_kernel<<<dim3(grid_for(nbins, KDE_THREADS), nblk[c]), KDE_THREADS, 0, cx.stream>>>(cls_x[c], cnt_u[c], mn, step,
                                                                                                   nbins, bw[c], pdf_partial[c].p);
    }
    kde_finish_kernel<<<1, 1024, 0, cx.stream>>>(pdf_partial[0].p, nblk[0], pdf_partial[1].p, nblk[1], nbins, constant[0],
                                                constant[1], pi, monotonic ? 1 : 0, fit.bins.p);
    HIP_TRY(hipGetLastError());
    fit.dev = KdeDev{fit.bins.p, mn, step, nbins};
    return true;
}

// one rung of Gauss::solve's epsilon ladder (gauss.rs:54-165) for the 20 x 20 system, and for the D x D systems of rt_model.hip
bool gauss_attempt(Dense left, Dense right, double eps, std::vector<double>& out) {
    const size_t m = left.rows, n = left.cols;
    for (size_t i = 0; i < n; ++i) left.at(i, i) += eps;  // fill_zero, :62-66
    size_t h = 0, k = 0;                                  // echelon, :89-124
    while (h < m && k < n) {
        size_t piv = 0;
        double best = std::numeric_limits<double>::lowest();
        for (size_t i = h; i < m; ++i)
            if (left.at(i, k) >= best) {
                piv = i;
                best = left.at(i, k);
            }
        if (left.at(piv, k) == 0.0) {
            ++k;
            continue;
        }
        if (h != piv) {
            left.swap_rows(h, piv);
            right.swap_rows(h, piv);
        }
        for (size_t i = h + 1; i < m; ++i) {
            const double factor = left.at(i, k) / left.at(h, k);
            left.at(i, k) = 0.0;
            for (size_t j = k + 1; j < n; ++j) left.at(i, j) -= left.at(h, j) * factor;
            for (size_t j = 0; j < right.cols; ++j) right.at(i, j) -= right.at(h, j) * factor;
        }
        ++h;
        ++k;
    }
    for (size_t i = m; i-- > 0;)  // reduce, :127-143
        for (size_t j = 0; j < n; ++j) {
            const double x = left.at(i, j);
            if (x == 0.0) continue;
            for (size_t c = j; c < n; ++c) left.at(i, c) /= x;
            for (size_t c = 0; c < right.cols; ++c) right.at(i, c) /= x;
            break;
        }
    for (size_t i = m; i-- > 0;)  // backfill, :146-164
        for (size_t j = 0; j < n; ++j) {
            if (left.at(i, j) == 0.0) continue;
            for (size_t r = 0; r < i; ++r) {
                const double factor = left.at(r, j) / left.at(i, j);
                for (size_t c = 0; c < n; ++c) left.at(r, c) -= left.at(i, c) * factor;
                for (size_t c = 0; c < right.cols; ++c) right.at(r, c) -= right.at(i, c) * factor;
            }
            break;
        }
    for (size_t i = 0; i < n; ++i)  // left_solved, :69-87
        for (size_t j = 0; j < n; ++j) {
            const double x = left.at(i, j);
            if (i == j) {
                if (x != 1.0 && x != 0.0) return false;
            } else if (x > 1e-8) {
                return false;
            }
        }
    out = right.a;
    return true;
}

// descending stable sort of `n` f32 scores given as total-order keys; order_out[j] = index of the j-th best
bool sort_desc(Ctx& cx, uint32_t* d_keys_in, uint32_t* d_idx_in, uint32_t n, uint32_t* d_keys_out, uint32_t* d_idx_out) {
    Buf<uint8_t> temp;
    HIP_TRY(with_scratch(temp, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs_desc(t, b, d_keys_in, d_keys_out, d_idx_in, d_idx_out, n, 0, 32, cx.stream); }));
    HIP_TRY(hipStreamSynchronize(cx.stream));
    return true;
}

// out[j] = min(q[j], q[j + 1], ..., q[n - 1]): the reverse cumulative minimum of qvalue.rs:27-35 / fdr.rs:104-112
bool suffix_min(Ctx& cx, const float* d_q, float* d_out, uint32_t n) {
    if (n == 0) return true;
    auto in = rocprim::make_reverse_iterator(d_q + n);
    auto out = rocprim::make_reverse_iterator(d_out + n);
    Buf<uint8_t> temp;
    HIP_TRY(with_scratch(temp, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, in, out, (size_t)n, OpFmin(), cx.stream); }));
    HIP_TRY(hipStreamSynchronize(cx.stream));
    return true;
}

}  // namespace

// ---- exported to rt_model.hip and protein_groups.hip (post_search.h) ---------------------------------------------------------

ScratchScope::ScratchScope(int device, hipStream_t stream) {
    tl_stream = stream;
    tl_pooled = false;
    if (const char* e = getenv("SAGE_HIP_NO_POOL"))
        if (atoi(e) != 0) return;
    static bool configured[64] = {};
    hipMemPool_t pool = nullptr;
    if (hipDeviceGetDefaultMemPool(&pool, device) != hipSuccess || !pool) {
        (void)hipGetLastError();
        return;
    }
    if (device >= 0 && device < 64 && !configured[device]) {
        uint64_t keep = ~0ull;
        if (hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        configured[device] = true;
    }
    tl_pooled = true;
}
ScratchScope::~ScratchScope() {
    tl_stream = nullptr;
    tl_pooled = false;
}

hipError_t scratch_alloc(void** p, size_t bytes, hipStream_t* pool_stream) {
    if (tl_pooled) {
        if (hipMallocAsync(p, bytes, tl_stream) == hipSuccess) {
            *pool_stream = tl_stream;
            return hipSuccess;
        }
        (void)hipGetLastError();
        *p = nullptr;
    }
    *pool_stream = nullptr;
    return hipMalloc(p, bytes);
}

bool gauss_solve(const Dense& left, const Dense& right, std::vector<double>& out) {  // :43-52
    for (double eps = 1e-8; eps <= 1.0; eps *= 10.0)
        if (gauss_attempt(left, right, eps, out)) return true;
    return false;
}

// out[j] = sum of flags[0..j]
bool prefix_count(Ctx& cx, const uint32_t* d_flags, uint32_t* d_out, uint32_t n) {
    Buf<uint8_t> temp;
    HIP_TRY(with_scratch(temp, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, d_flags, d_out, (size_t)n, rocprim::plus<uint32_t>(), cx.stream); }));
    HIP_TRY(hipStreamSynchronize(cx.stream));
    return true;
}

// out[j] = sum of flags[0..j)
bool exclusive_count(Ctx& cx, const uint32_t* d_flags, uint32_t* d_out, uint64_t n) {
    Buf<uint8_t> temp;
    HIP_TRY(with_scratch(temp, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, d_flags, d_out, 0u, (size_t)n, rocprim::plus<uint32_t>(), cx.stream); }));
    return true;
}

// qvalue.rs:8-36 on the sorted order: decoy flags, their prefix count, q from the counts, the reverse cumulative minimum, and the
// scatter back to input order; the passing count reads the sorted q-values in between
bool spectrum_q_values(Ctx& cx, const uint32_t* d_order, const uint8_t* d_decoy, uint32_t n, uint32_t* d_flags, uint32_t* d_cum,
                       float* d_q_sorted, float* d_qmin_sorted, float* d_q_out, unsigned long long* d_passing) {
    const uint32_t g = grid_for(n, RB);
    decoy_flags_kernel<<<g, RB, 0, cx.stream>>>(d_order, d_decoy, n, d_flags);
    if (!prefix_count(cx, d_flags, d_cum, n)) return false;
    q_from_counts_kernel<<<g, RB, 0, cx.stream>>>(d_cum, n, d_q_sorted);
    if (!suffix_min(cx, d_q_sorted, d_qmin_sorted, n)) return false;
    if (d_passing) {
        HIP_TRY(hipMemsetAsync(d_passing, 0, 8, cx.stream));
        count_passing_kernel<<<g, RB, 0, cx.stream>>>(d_qmin_sorted, n, nullptr, 0.01f, d_passing);
    }
    scatter_by_order_kernel<<<g, RB, 0, cx.stream>>>(d_order, d_qmin_sorted, n, d_q_out);
    return true;
}

// Competition::assign_q_value over dense keys (fdr.rs:60-120) and the write-back of fdr.rs:146-148 / :179-185
bool picked(Ctx& cx, const uint32_t* d_key, uint32_t n_keys, const uint8_t* d_decoy, const float* d_score, uint64_t n,
            float* d_q_out, uint64_t& passing) {
    passing = 0;
    if (n_keys == 0) {  // no feature takes part: every q stays 1.0
        Buf<float> dummy;
        HIP_TRY(dummy.alloc(2));
        picked_gather_kernel<<<grid_for(n, RB), RB, 0, cx.stream>>>(d_key, d_decoy, n, dummy.p, d_q_out);
        HIP_TRY(hipStreamSynchronize(cx.stream));
        return true;
    }
    const uint32_t n_rows = 2 * n_keys;
    Buf<uint32_t> side, row_key, row_id, sorted_key, sorted_id, counters;
    Buf<double> winner;
    Buf<uint8_t> winner_decoy, row_decoy;
    Buf<float> pep, dsum, q, qmin, side_q;
    Buf<uint32_t> target_flag, target_cum;
    Buf<unsigned long long> d_pass;
    HIP_TRY(side.alloc(n_rows));
    HIP_TRY(row_key.alloc(n_rows));
    HIP_TRY(row_id.alloc(n_rows));
    HIP_TRY(sorted_key.alloc(n_rows));
    HIP_TRY(sorted_id.alloc(n_rows));
    HIP_TRY(counters.alloc(2));
    HIP_TRY(winner.alloc(n_keys));
    HIP_TRY(winner_decoy.alloc(n_keys));
    HIP_TRY(row_decoy.alloc(n_rows));
    HIP_TRY(pep.alloc((size_t)n_rows + CS_TILE));
    HIP_TRY(dsum.alloc((size_t)n_rows + CS_TILE));
    HIP_TRY(q.alloc(n_rows));
    HIP_TRY(qmin.alloc(n_rows));
    HIP_TRY(target_flag.alloc(n_rows));
    HIP_TRY(target_cum.alloc(n_rows));
    HIP_TRY(side_q.alloc(n_rows));
    HIP_TRY(d_pass.alloc(1));
    HIP_TRY(hipMemsetAsync(side.p, 0, (size_t)n_rows * 4, cx.stream));
    HIP_TRY(hipMemsetAsync(counters.p, 0, 8, cx.stream));
    picked_max_kernel<<<grid_for(n, RB), RB, 0, cx.stream>>>(d_key, d_decoy, d_score, n, side.p);
    picked_rows_kernel<<<grid_for(n_keys, RB), RB, 0, cx.stream>>>(side.p, n_keys, winner.p, winner_decoy.p, row_key.p, row_id.p,
                                                                    counters.p);
    uint32_t h_counters[2];
    HIP_TRY(hipMemcpyAsync(h_counters, counters.p, 8, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipStreamSynchronize(cx.stream));
    if (h_counters[1]) {
        return cx.fail(SAGE_HIP_ERR_INVALID, "sage_hip_rescore: competition keys must be dense (" + std::to_string(h_counters[1]) + " of " +
                                                 std::to_string(n_keys) + " ids are not used by any feature)");
    }
    const uint32_t m = h_counters[0];
    KdeFit est;
    if (!kde_build(cx, winner.p, winner_decoy.p, n_keys, true, 1000, 1.0, est)) return false;
    if (!sort_desc(cx, row_key.p, row_id.p, n_rows, sorted_key.p, sorted_id.p)) return false;  // absent rows (key 0) sort last
    const uint32_t m_padded = (m + CS_TILE - 1u) / CS_TILE * CS_TILE;
    picked_pep_kernel<<<grid_for(m_padded, RB), RB, 0, cx.stream>>>(sorted_key.p, sorted_id.p, m, m_padded, est.dev, pep.p,
                                                                     row_decoy.p, target_flag.p);
    if (!prefix_count(cx, target_flag.p, target_cum.p, m)) return false;
    seq_cumsum_kernel<<<1, 64, 0, cx.stream>>>(pep.p, m_padded, dsum.p);
    picked_q_kernel<<<grid_for(m, RB), RB, 0, cx.stream>>>(dsum.p, target_cum.p, m, q.p);
    if (!suffix_min(cx, q.p, qmin.p, m)) return false;
    HIP_TRY(hipMemsetAsync(d_pass.p, 0, 8, cx.stream));
    count_passing_kernel<<<grid_for(m, RB), RB, 0, cx.stream>>>(qmin.p, m, row_decoy.p, 0.01f, d_pass.p);
    // rows that do not exist keep q = 1.0 (never read: a feature's own side always exists)
    std::vector<float> ones(n_rows, 1.0f);
    HIP_TRY(hipMemcpyAsync(side_q.p, ones.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, cx.stream));
    picked_scatter_kernel<<<grid_for(m, RB), RB, 0, cx.stream>>>(sorted_id.p, qmin.p, m, side_q.p);
    picked_gather_kernel<<<grid_for(n, RB), RB, 0, cx.stream>>>(d_key, d_decoy, n, side_q.p, d_q_out);
    unsigned long long h_pass = 0;
    HIP_TRY(hipMemcpyAsync(&h_pass, d_pass.p, 8, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(cx.stream));
    passing = h_pass;
    return true;
}

namespace {

bool rescore_impl(Ctx& cx, const SageRescoreInput& in, SageRescoreOutput& out) {
    const uint64_t n = in.n;
    const int tol_kind = in.precursor_tol.kind;
    Buf<SageFeature> feats;
    Buf<uint8_t> decoy;
    Buf<double> dmass, rows, disc, partial, folded;
    Buf<float> a_rt, d_rt, d_ims, discriminant, posterior, spectrum_q, peptide_q, protein_q, qsorted, qmin_sorted;
    Buf<uint32_t> pkey, prkey, keys, idx, keys_sorted, order;
    Buf<unsigned long long> d_pass;
    HIP_TRY(feats.alloc(n));
    HIP_TRY(decoy.alloc(n));
    HIP_TRY(dmass.alloc(n));
    HIP_TRY(rows.alloc(n * NF));
    HIP_TRY(disc.alloc(n));
    HIP_TRY(discriminant.alloc(n));
    HIP_TRY(posterior.alloc(n));
    HIP_TRY(spectrum_q.alloc(n));
    HIP_TRY(peptide_q.alloc(n));
    HIP_TRY(protein_q.alloc(n));
    HIP_TRY(qsorted.alloc(n));
    HIP_TRY(qmin_sorted.alloc(n));
    HIP_TRY(pkey.alloc(n));
    HIP_TRY(prkey.alloc(n));
    HIP_TRY(keys.alloc(n));
    HIP_TRY(idx.alloc(n));
    HIP_TRY(keys_sorted.alloc(n));
    HIP_TRY(order.alloc(n));
    HIP_TRY(d_pass.alloc(1));
    HIP_TRY(hipMemcpyAsync(feats.p, in.features, n * sizeof(SageFeature), hipMemcpyHostToDevice, cx.stream));
    HIP_TRY(hipMemcpyAsync(pkey.p, in.peptide_key, n * 4, hipMemcpyHostToDevice, cx.stream));
    HIP_TRY(hipMemcpyAsync(prkey.p, in.protein_key, n * 4, hipMemcpyHostToDevice, cx.stream));
    const float* opt[3] = {in.aligned_rt, in.delta_rt_model, in.delta_ims_model};
    Buf<float>* optbuf[3] = {&a_rt, &d_rt, &d_ims};
    for (int k = 0; k < 3; ++k)
        if (opt[k]) {
            HIP_TRY(optbuf[k]->alloc(n));
            HIP_TRY(hipMemcpyAsync(optbuf[k]->p, opt[k], n * 4, hipMemcpyHostToDevice, cx.stream));
        }
    Events<2> ev;  // start, stop
    HIP_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev[0], cx.stream));
    const uint32_t g = grid_for(n, RB);
    prep_kernel<<<g, RB, 0, cx.stream>>>(feats.p, n, tol_kind, decoy.p, dmass.p);

    // ---- score_psms (linear_discriminant.rs:133-231) ----
    const double bw_adjust = tol_kind == SAGE_TOL_PPM ? 2.0 : 0.1;  // :146-150
    const float span = in.precursor_tol.hi - in.precursor_tol.lo;
    const float bin_size = tol_kind == SAGE_TOL_PPM ? std::fmax(span, 100.0f) : std::fmax(span, 1000.0f);
    const uint32_t mass_bins = (uint32_t)std::fabs(std::ceil(bin_size));
    KdeFit mass_model;
    if (!kde_build(cx, dmass.p, decoy.p, n, false, mass_bins, bw_adjust, mass_model)) return false;
    rows_kernel<<<g, RB, 0, cx.stream>>>(feats.p, n, dmass.p, mass_model.dev, a_rt.p, d_rt.p, d_ims.p, rows.p);

    // train (:57-127): class sums -> means -> scatter -> solve; both passes in the reference's row order (seq_lda_kernel)
    HIP_TRY(folded.alloc(2 * NF * NF + 2 * NF));
    seq_lda_kernel<false><<<dim3(1, 2), SEQ_THREADS, 0, cx.stream>>>(rows.p, decoy.p, n, nullptr, folded.p);
    double class_sum[2][NF];
    HIP_TRY(hipMemcpyAsync(class_sum, folded.p, sizeof(class_sum), hipMemcpyDeviceToHost, cx.stream));
    // class counts: the decoy flags summed by the mass-model fit would do; recount on the host from the labels instead
    HIP_TRY(hipStreamSynchronize(cx.stream));
    uint64_t class_count[2] = {0, 0};
    for (uint64_t i = 0; i < n; ++i) class_count[in.features[i].label == -1 ? 0 : 1]++;
    bool fitted = class_count[0] != 0 && class_count[1] != 0;  // :83-85
    std::vector<double> coef;
    if (fitted) {
        double class_mean[2][NF];
        for (int c = 0; c < 2; ++c)
            for (int j = 0; j < NF; ++j) class_mean[c][j] = class_sum[c][j] / (double)class_count[c];
        double* d_mean = folded.p + 2 * NF * NF;
        HIP_TRY(hipMemcpyAsync(d_mean, class_mean, sizeof(class_mean), hipMemcpyHostToDevice, cx.stream));
        seq_lda_kernel<true><<<dim3(1, 2), SEQ_THREADS, 0, cx.stream>>>(rows.p, decoy.p, n, d_mean, folded.p);
        std::vector<double> scatter(2 * NF * NF);
        HIP_TRY(hipMemcpyAsync(scatter.data(), folded.p, scatter.size() * 8, hipMemcpyDeviceToHost, cx.stream));
        HIP_TRY(hipStreamSynchronize(cx.stream));
        Dense within(NF, NF), mu(NF, 1);
        for (int c = 0; c < 2; ++c)  // :105-108
            for (int e = 0; e < NF * NF; ++e) within.a[e] += scatter[c * NF * NF + e] / (double)class_count[c];
        for (int j = 0; j < NF; ++j) mu.a[j] = class_mean[1][j] - class_mean[0][j];
        fitted = gauss_solve(within, mu, coef);
        if (fitted)
            for (double c : coef)
                if (!std::isfinite(c)) fitted = false;  // :198-210
    }
    out.lda_fitted = fitted ? 1 : 0;
    std::memset(out.coef, 0, sizeof(out.coef));
    KdeFit kde;
    if (fitted) {
        Coef cf;
        for (int j = 0; j < NF; ++j) out.coef[j] = cf.w[j] = coef[j];
        project_kernel<<<g, RB, 0, cx.stream>>>(rows.p, n, cf, disc.p);
        if (!kde_build(cx, disc.p, decoy.p, n, true, 1000, 1.0, kde)) return false;
        pep_kernel<<<g, RB, 0, cx.stream>>>(disc.p, n, kde.dev, discriminant.p, posterior.p);
    } else {
        heuristic_kernel<<<g, RB, 0, cx.stream>>>(feats.p, n, discriminant.p, posterior.p);
    }

    // ---- runner.rs:290-291: sort by discriminant, spectrum_q_value ----
    sort_keys_kernel<<<g, RB, 0, cx.stream>>>(discriminant.p, (uint32_t)n, keys.p, idx.p);
    if (!sort_desc(cx, keys.p, idx.p, (uint32_t)n, keys_sorted.p, order.p)) return false;
    if (!spectrum_q_values(cx, order.p, decoy.p, (uint32_t)n, keys.p, idx.p, qsorted.p, qmin_sorted.p, spectrum_q.p, d_pass.p))
        return false;  // (keys / idx are free again: its scratch)
    unsigned long long h_pass = 0;
    HIP_TRY(hipMemcpyAsync(&h_pass, d_pass.p, 8, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(cx.stream));
    out.passing_spectrum = h_pass;

    // ---- fdr.rs:123-187 ----
    if (!picked(cx, pkey.p, in.n_peptide_keys, decoy.p, discriminant.p, n, peptide_q.p, out.passing_peptide)) return false;
    if (!picked(cx, prkey.p, in.n_protein_keys, decoy.p, discriminant.p, n, protein_q.p, out.passing_protein)) return false;
    HIP_TRY(hipEventRecord(ev[1], cx.stream));

    HIP_TRY(hipMemcpyAsync(out.discriminant_score, discriminant.p, n * 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(out.posterior_error, posterior.p, n * 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(out.spectrum_q, spectrum_q.p, n * 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(out.peptide_q, peptide_q.p, n * 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipMemcpyAsync(out.protein_q, protein_q.p, n * 4, hipMemcpyDeviceToHost, cx.stream));
    if (out.order) HIP_TRY(hipMemcpyAsync(out.order, order.p, n * 4, hipMemcpyDeviceToHost, cx.stream));
    HIP_TRY(hipStreamSynchronize(cx.stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    out.device_ms = ms;
    return true;
}

}  // namespace

// entry point used by capi_host.cpp; returns a SAGE_HIP_* status, message in `err`
int rescore_on_device(int device, const SageRescoreInput& in, SageRescoreOutput& out, std::string& err) {
    return run_on_device<ScratchScope>(device, "sage_hip_rescore", "", err, [&](Ctx& cx) { return rescore_impl(cx, in, out); });
}

}  // namespace sagehip
