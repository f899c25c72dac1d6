// maxlfq.h — the arithmetic of the protein-level roll-up of label-free quantification (MaxLFQ), shared by the
// device (protein_lfq.hip) and the host (tests/hostemu/maxlfq_emu.cpp compiles it by itself): the logarithm of a cell, the
// order-preserving key of a difference, the exact selection of a median by its bits, and — as ONE function over a `Team` —
// components, normal equations, elimination, back substitution and anchor of one protein.  A Team is whoever runs the function
// together: a workgroup on the device (rank = thread, sync = barrier), a single caller on the host (SerialTeam).  Every value
// the function stores is defined by DESIGN.md 7g alone, so it does not depend on which member computes it.
//
// All arithmetic is IEEE f64 without contraction (-ffp-contract=off on every translation unit that includes this file).
#pragma once
#include <stdint.h>

#include "crlog.h"
#include "detmath.h"

namespace maxlfq {

constexpr uint32_t NONE = 0xFFFFFFFFu;   // protein_of_row: the row is ignored; component: the file is not quantified
constexpr uint32_t MAX_FILES = 65535u;

SAGE_HD uint64_t bits_of(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    return u;
}
SAGE_HD double double_of(uint64_t u) {
    double v;
    __builtin_memcpy(&v, &u, 8);
    return v;
}
SAGE_HD double missing() { return double_of(0x7ff8000000000000ull); }
SAGE_HD bool present(double l) { return l == l; }

// step 1: the natural log of an area that is a positive finite number, else missing
SAGE_HD double log_of_area(double area) { return (area > 0.0 && area < __builtin_inf()) ? sagecore::cr_log(area) : missing(); }

// step 2: a difference as a u64 whose unsigned order is the order of the doubles (differences of two finite logs are finite and
// never -0.0, so the order is total and the median's bits do not depend on the selection method)
SAGE_HD uint64_t key_of(double d) {
    const uint64_t u = bits_of(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
SAGE_HD double of_key(uint64_t k) { return double_of((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k); }
// the median of `count` >= 1 values from the elements of rank (count - 1) / 2 and count / 2 in ascending order
SAGE_HD double median_of(double lo, double hi, uint32_t count) { return (count & 1u) ? lo : (lo + hi) * 0.5; }
// position of the pair (j, k), j < k < n, in lexicographic order
SAGE_HD uint64_t pair_index(uint32_t j, uint32_t k, uint32_t n) {
    return (uint64_t)j * n - (uint64_t)j * (j + 1) / 2 + (k - j - 1);
}
SAGE_HD uint64_t n_pairs(uint32_t n) { return (uint64_t)n * (n - (n ? 1 : 0)) / 2; }

// The key of rank `rank` (0-based, ascending) among a multiset of keys, one bit at a time from the top.  zeros(prefix, bit): how
// many keys agree with `prefix` in the bits above `bit` and have bit `bit` clear.  Exact, and uniform for everyone who calls it
// with the same counts.
template <class Zeros>
SAGE_HD uint64_t radix_select(uint32_t rank, Zeros zeros) {
    uint64_t prefix = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const uint32_t z = zeros(prefix, bit);
        if (rank >= z) {
            rank -= z;
            prefix |= 1ull << bit;
        }
    }
    return prefix;
}

struct SerialTeam {
    SAGE_HD uint32_t rank() const { return 0; }
    SAGE_HD uint32_t size() const { return 1; }
    SAGE_HD void sync() const {}
    SAGE_HD bool any(bool mine) const { return mine; }
};

// step 6, first half: col[j] = sum of the present L[r][j] from +0.0 in ascending r, ncol[j] their number.  L is file-major:
// the cell of (row r of this protein, file j) is L[j * stride + r], r in [0, n_rows).
template <class Team>
SAGE_HD void column_sums(const Team& t, const double* L, uint64_t stride, uint32_t n_rows, uint32_t n, double* col, uint32_t* ncol) {
    for (uint32_t j = t.rank(); j < n; j += t.size()) {
        const double* c = L + (uint64_t)j * stride;
        double s = 0.0;
        uint32_t m = 0;
        for (uint32_t r = 0; r < n_rows; ++r) {
            const double l = c[r];
            if (present(l)) {
                s = s + l;
                ++m;
            }
        }
        col[j] = s;
        ncol[j] = m;
    }
}

// One protein between its pair tables and its results.
struct Protein {
    uint32_t n;           // files
    uint32_t min_count;   // max(min_ratio_count, 1)
    const double* med;    // [n (n - 1) / 2] pair medians (read where cnt >= min_count)
    const uint32_t* cnt;  // [n (n - 1) / 2] shared rows of a pair
    const double* col;    // [n] column_sums
    const uint32_t* ncol;
    double* A;            // [n * (n + 1)] the augmented matrix, row stride n + 1, b in column n (scratch)
    double* f;            // [n] the factors of one elimination step, then the anchors of the components (scratch)
    double* x;            // [n] out: log abundance (NaN: not quantified)
    double* intensity;    // [n] out: det_exp(x), 0.0 where not quantified
    uint32_t* label;      // [n] out: component label (NONE where not quantified)
};

// steps 3-7.  Returns 0, or 1 + p when pivot p is zero or not finite (every member returns the same value).
template <class Team>
SAGE_HD uint32_t solve(const Team& t, const Protein& v, uint32_t* n_components) {
    const uint32_t n = v.n, R = t.rank(), S = t.size(), W = n + 1, mc = v.min_count;
    // 3. components: every file takes the smallest label among its valid neighbours until nothing changes.  The labels only
    // decrease and the fixed point — the smallest file index of the component — is unique, so a label read while its owner
    // lowers it (the old or the new value) changes how many sweeps it takes, not where they end.
    for (uint32_t j = R; j < n; j += S) v.label[j] = j;
    t.sync();
    for (;;) {
        bool changed = false;
        for (uint32_t j = R; j < n; j += S) {
            uint32_t m = v.label[j];
            for (uint32_t k = 0; k < n; ++k) {
                if (k == j || v.cnt[j < k ? pair_index(j, k, n) : pair_index(k, j, n)] < mc) continue;
                const uint32_t l = v.label[k];
                if (l < m) m = l;
            }
            if (m < v.label[j]) {
                v.label[j] = m;
                changed = true;
            }
        }
        if (!t.any(changed)) break;
    }
    // 4. normal equations, row by row; a file that is its component's label is grounded
    for (uint32_t j = R; j < n; j += S) {
        double* row = v.A + (uint64_t)j * W;
        const bool grounded = v.label[j] == j;
        double degree = 0.0, b = 0.0;
        for (uint32_t k = 0; k < n; ++k) {
            double a = 0.0;
            if (k != j) {
                const uint64_t q = j < k ? pair_index(j, k, n) : pair_index(k, j, n);
                if (v.cnt[q] >= mc) {
                    const double m = v.med[q];
                    degree = degree + 1.0;
                    a = -1.0;
                    b = j < k ? b + m : b - m;
                }
            }
            row[k] = (grounded || v.label[k] == k) ? 0.0 : a;
        }
        row[j] = grounded ? 1.0 : degree;
        row[n] = grounded ? 0.0 : b;
    }
    t.sync();
    // 5. forward elimination without pivoting.  The factors of a step are taken before any entry of the step changes (column p
    // of a row is itself updated); a row whose entry in the pivot column is 0.0 is left untouched (f: NaN).
    for (uint32_t p = 0; p < n; ++p) {
        const double pivot = v.A[(uint64_t)p * W + p];
        if (!(pivot != 0.0 && pivot - pivot == 0.0)) return 1 + p;
        for (uint32_t i = p + 1 + R; i < n; i += S) {
            const double a = v.A[(uint64_t)i * W + p];
            v.f[i] = a == 0.0 ? missing() : a / pivot;
        }
        t.sync();
        const uint32_t cols = W - p, cells = (n - 1 - p) * cols;  // (< 2^32 for n <= 65535)
        const double* prow = v.A + (uint64_t)p * W;
        for (uint32_t e = R; e < cells; e += S) {
            const uint32_t i = p + 1 + e / cols, c = p + e % cols;
            const double f = v.f[i];
            if (f == f) {
                double* cell = v.A + (uint64_t)i * W + c;
                *cell = *cell - f * prow[c];
            }
        }
        t.sync();
    }
    // back substitution: one chain, in the order of the contract
    if (R == 0) {
        for (uint32_t i = n; i-- > 0;) {
            const double* row = v.A + (uint64_t)i * W;
            double s = row[n];
            for (uint32_t c = i + 1; c < n; ++c) s = s - row[c] * v.x[c];
            v.x[i] = s / row[i];
        }
    }
    t.sync();
    // 6. anchor: the component's label adds up its members in ascending order
    for (uint32_t j = R; j < n; j += S) {
        if (v.label[j] != j) continue;
        double T = 0.0, X = 0.0;
        uint64_t N = 0;
        uint32_t members = 0;
        for (uint32_t m = j; m < n; ++m) {
            if (v.label[m] != j) continue;
            T = T + v.col[m];
            N += v.ncol[m];
            X = X + v.x[m];
            ++members;
        }
        v.f[j] = N ? T / (double)N - X / (double)members : missing();
    }
    t.sync();
    if (R == 0) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < n; ++j) c += (v.label[j] == j && present(v.f[j])) ? 1u : 0u;
        *n_components = c;
    }
    t.sync();
    // 7. results (a member reads only its own label here, and the anchors, which no one writes any more)
    for (uint32_t j = R; j < n; j += S) {
        const double d = v.f[v.label[j]];
        if (present(d)) {
            const double y = v.x[j] + d;
            v.x[j] = y;
            v.intensity[j] = sagedet::det_exp(y);
        } else {
            v.x[j] = missing();
            v.intensity[j] = 0.0;
            v.label[j] = NONE;
        }
    }
    t.sync();
    return 0;
}

}  // namespace maxlfq
