// tmt_rollup_emu.cpp — sage_amd/csrc/tmt_rollup.h compiled for the host: the roll-up of DESIGN.md 7i by one caller, over the layout
// the device uses (used rows grouped stably, centred logs channel-major).  Built as a shared library by tests/test_tmt_rollup_cpu.py
// and held bit for bit to tests/tmt_rollup_reference.py.
#include <algorithm>
#include <vector>

#include "../../sage_amd/csrc/tmt_rollup.h"

// Returns 0; 1: a group id out of range, or normalise / summary unknown.
extern "C" int emu_tmt_rollup(uint64_t n_rows, uint32_t n, uint32_t n_groups, uint32_t min_present, int normalise, int summary,
                              const float* intensity, const uint32_t* group_of_row, double* abundance, double* log_abundance,
                              uint32_t* n_cells, uint32_t* n_rows_used, double* factor, double* column_sum, uint64_t* n_used_rows) {
    if (normalise < 0 || normalise > 1 || summary < 0 || summary > 1) return 1;
    const uint32_t need = tmtroll::needed(min_present);
    std::vector<uint32_t> key(n_rows);
    std::vector<uint64_t> off((size_t)n_groups + 1, 0);
    for (uint64_t r = 0; r < n_rows; ++r) {
        const uint32_t g = group_of_row[r];
        if (g != tmtroll::NONE && g >= n_groups) return 1;
        const bool used = g != tmtroll::NONE && tmtroll::present_cells(intensity + r * n, n) >= need;
        key[r] = used ? g : tmtroll::NONE;
        if (used) ++off[(size_t)g + 1];
    }
    for (uint32_t g = 0; g < n_groups; ++g) {
        n_rows_used[g] = (uint32_t)off[(size_t)g + 1];
        off[(size_t)g + 1] += off[g];
    }
    const uint64_t n_used = off[n_groups];
    *n_used_rows = n_used;
    // grouped order (ascending r: the grouping is stable)
    std::vector<uint64_t> next(off.begin(), off.end() - 1), row(n_used);
    for (uint64_t r = 0; r < n_rows; ++r)
        if (key[r] != tmtroll::NONE) row[next[key[r]]++] = r;
    // column sums and factors
    const uint32_t n_blocks = (uint32_t)((n_rows + tmtroll::BLOCK_ROWS - 1) / tmtroll::BLOCK_ROWS);
    std::vector<double> P((size_t)n_blocks * n);
    std::vector<uint32_t> PC((size_t)n_blocks * n), C(n);
    for (uint32_t b = 0; b < n_blocks; ++b)
        for (uint32_t k = 0; k < n; ++k) {
            const uint64_t lo = (uint64_t)b * tmtroll::BLOCK_ROWS, hi = std::min<uint64_t>(lo + tmtroll::BLOCK_ROWS, n_rows);
            tmtroll::block_partial(intensity, n, k, lo, hi, [&](uint64_t r) { return key[r] != tmtroll::NONE; }, &P[(size_t)b * n + k],
                                   &PC[(size_t)b * n + k]);
        }
    for (uint32_t k = 0; k < n; ++k) tmtroll::fold_partials(P.data(), PC.data(), n_blocks, n, k, column_sum + k, &C[k]);
    const double M = tmtroll::mean_column_sum(column_sum, C.data(), n);
    for (uint32_t k = 0; k < n; ++k) factor[k] = tmtroll::factor_of(normalise, M, column_sum[k], C[k]);
    // summaries
    std::vector<double> D, centre;
    if (summary == tmtroll::SUMMARY_MEDIAN) {
        D.resize((size_t)n_used * n);
        centre.resize(n_used);
        for (uint64_t i = 0; i < n_used; ++i) {
            const double c = tmtroll::row_centre(intensity + row[i] * n, factor, n, [&](uint32_t k, double l) { D[(size_t)k * n_used + i] = l; });
            centre[i] = c;
            for (uint32_t k = 0; k < n; ++k) D[(size_t)k * n_used + i] = D[(size_t)k * n_used + i] - c;
        }
    }
    std::vector<uint64_t> keys;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint64_t a = off[g];
        const uint32_t nr = (uint32_t)(off[(size_t)g + 1] - a);
        const double ag = (summary == tmtroll::SUMMARY_MEDIAN && nr) ? tmtroll::group_centre(centre.data() + a, nr) : maxlfq::missing();
        for (uint32_t k = 0; k < n; ++k) {
            const uint64_t o = (uint64_t)g * n + k;
            if (summary == tmtroll::SUMMARY_SUM) {
                double s = 0.0;
                uint32_t c = 0;
                for (uint32_t i = 0; i < nr; ++i) {
                    const float x = intensity[row[a + i] * n + k];
                    if (tmtroll::present(x)) {
                        s = s + tmtroll::weighted(x, factor[k]);
                        ++c;
                    }
                }
                tmtroll::finish_sum(s, c, abundance + o, log_abundance + o);
                n_cells[o] = c;
                continue;
            }
            keys.clear();
            for (uint32_t i = 0; i < nr; ++i) {
                const double d = D[(size_t)k * n_used + a + i];
                if (maxlfq::present(d)) keys.push_back(maxlfq::key_of(d));
            }
            const uint32_t c = (uint32_t)keys.size();
            uint64_t lo = 0, hi = 0;
            if (c) {
                auto zeros = [&](uint64_t prefix, int bit) {
                    uint32_t z = 0;
                    for (uint64_t key : keys) z += (key >> bit) == (prefix >> bit) ? 1u : 0u;
                    return z;
                };
                lo = maxlfq::radix_select((c - 1) / 2, zeros);
                hi = maxlfq::radix_select(c / 2, zeros);
            }
            tmtroll::finish_median(lo, hi, c, ag, abundance + o, log_abundance + o);
            n_cells[o] = c;
        }
    }
    return 0;
}
