// tmt_rollup.h — the arithmetic of the roll-up of TMT reporter intensities to one abundance per group and channel,
// shared by the device (tmt_rollup.hip) and the host (tests/hostemu/tmt_rollup_emu.cpp compiles it by itself): what a present cell
// is, the block partials of the column sums and their fold, the loading factors, the centre of a row, and how a group's channel is
// finished from its sum or from the two middle keys of its centred logs.  Every function is sequential in the order the contract
// names; who calls it for which row, channel or group is the caller's business.  The median's keys and their exact selection are
// maxlfq.h's (key_of, radix_select, median_of).
//
// All arithmetic is IEEE f64 without contraction (-ffp-contract=off on every translation unit that includes this file).
#pragma once
#include <stdint.h>

#include "maxlfq.h"

namespace tmtroll {

constexpr uint32_t NONE = 0xFFFFFFFFu;    // group_of_row: the row is ignored
constexpr uint32_t MAX_LABELS = 65535u;
constexpr uint32_t BLOCK_ROWS = 1024u;    // input rows of one partial of the column sums
enum { NORMALISE_NONE = 0, NORMALISE_TOTAL = 1, SUMMARY_SUM = 0, SUMMARY_MEDIAN = 1 };

// step 1
SAGE_HD bool present(float x) {
    const double v = (double)x;
    return v > 0.0 && v < __builtin_inf();
}
SAGE_HD uint32_t needed(uint32_t min_present) { return min_present ? min_present : 1u; }
SAGE_HD uint32_t present_cells(const float* row, uint32_t n_labels) {
    uint32_t c = 0;
    for (uint32_t k = 0; k < n_labels; ++k) c += present(row[k]) ? 1u : 0u;
    return c;
}

// step 2: P[b][k] and the block's share of C[k] for channel k; `used(r)`: whether input row r is used
template <class Used>
SAGE_HD void block_partial(const float* intensity, uint32_t n_labels, uint32_t k, uint64_t row_begin, uint64_t row_end, Used used,
                           double* sum, uint32_t* cells) {
    double s = 0.0;
    uint32_t c = 0;
    for (uint64_t r = row_begin; r < row_end; ++r) {
        const float x = intensity[r * n_labels + k];
        if (used(r) && present(x)) {
            s = s + (double)x;
            ++c;
        }
    }
    *sum = s;
    *cells = c;
}
// S[k] and C[k] from the partials of channel k, ascending b (partials are [n_blocks * n_labels])
SAGE_HD void fold_partials(const double* P, const uint32_t* PC, uint32_t n_blocks, uint32_t n_labels, uint32_t k, double* S, uint32_t* C) {
    double s = 0.0;
    uint32_t c = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        s = s + P[(uint64_t)b * n_labels + k];
        c += PC[(uint64_t)b * n_labels + k];
    }
    *S = s;
    *C = c;
}

// step 3: M (1.0 when no channel has a present cell: never read then), and the factor of a channel
SAGE_HD double mean_column_sum(const double* S, const uint32_t* C, uint32_t n_labels) {
    double t = 0.0;
    uint32_t m = 0;
    for (uint32_t k = 0; k < n_labels; ++k)
        if (C[k] > 0) {
            t = t + S[k];
            ++m;
        }
    return m ? t / (double)m : 1.0;
}
SAGE_HD double factor_of(int normalise, double M, double S, uint32_t C) { return (normalise == NORMALISE_TOTAL && C > 0) ? M / S : 1.0; }
SAGE_HD double weighted(float x, double f) { return (double)x * f; }

// step 5: l of every cell of a row through store(k, l) (missing: NaN), and the row's centre.  The row has a present cell.
template <class Store>
SAGE_HD double row_centre(const float* row, const double* f, uint32_t n_labels, Store store) {
    double s = 0.0;
    uint32_t m = 0;
    for (uint32_t k = 0; k < n_labels; ++k) {
        double l = maxlfq::missing();
        if (present(row[k])) {
            l = sagecore::cr_log(weighted(row[k], f[k]));
            s = s + l;
            ++m;
        }
        store(k, l);
    }
    return s / (double)m;
}
// a[g]: centres of the group's used rows in ascending row index
SAGE_HD double group_centre(const double* c, uint32_t n_rows) {
    double s = 0.0;
    for (uint32_t r = 0; r < n_rows; ++r) s = s + c[r];
    return s / (double)n_rows;
}

// steps 4 and 5, last lines: one (group, channel) from its sum / from the keys of ranks (cells - 1) / 2 and cells / 2
SAGE_HD void finish_sum(double sum, uint32_t cells, double* abundance, double* log_abundance) {
    *abundance = cells ? sum : 0.0;
    *log_abundance = cells ? sagecore::cr_log(sum) : maxlfq::missing();
}
SAGE_HD void finish_median(uint64_t key_lo, uint64_t key_hi, uint32_t cells, double a, double* abundance, double* log_abundance) {
    if (!cells) {
        *abundance = 0.0;
        *log_abundance = maxlfq::missing();
        return;
    }
    const double y = maxlfq::median_of(maxlfq::of_key(key_lo), maxlfq::of_key(key_hi), cells) + a;
    *log_abundance = y;
    *abundance = sagedet::det_exp(y);
}

}  // namespace tmtroll
