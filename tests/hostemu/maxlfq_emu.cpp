// maxlfq_emu.cpp — sage_amd/csrc/maxlfq.h compiled for the host: the protein roll-up of DESIGN.md 7g with one caller as the Team
// (maxlfq::SerialTeam), over the layout the device uses (rows grouped by protein, stably; logs file-major).  Built two ways by
// tests/test_protein_lfq_cpu.py: as a shared library (emu_protein_lfq, held bit for bit to tests/protein_lfq_reference.py, and
// timed by scripts/protein_lfq_bench.py), and with -DMAXLFQ_EMU_MAIN as a program of its own under AddressSanitizer and
// UndefinedBehaviorSanitizer, which reads worlds from files:
//     u64 n_rows, u32 n_files, u32 n_proteins, u32 min_ratio_count, u32 0, f64 areas[n_rows * n_files], u32 protein_of_row[n_rows]
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sage_amd/csrc/maxlfq.h"

// Returns 0; 1: a protein id out of range; 2 + p: a zero or non-finite pivot in protein p.  pair_median / pair_count may be null.
extern "C" int emu_protein_lfq(uint64_t n_rows, uint32_t n, uint32_t n_proteins, uint32_t min_ratio_count, const double* areas,
                               const uint32_t* protein_of_row, double* log_abundance, double* intensity, uint32_t* component,
                               uint32_t* n_rows_used, uint32_t* n_components, double* pair_median, uint32_t* pair_count) {
    const uint32_t mc = min_ratio_count ? min_ratio_count : 1;
    const uint64_t P = maxlfq::n_pairs(n);
    std::vector<uint64_t> off((size_t)n_proteins + 1, 0);
    for (uint64_t r = 0; r < n_rows; ++r) {
        const uint32_t p = protein_of_row[r];
        if (p == maxlfq::NONE) continue;
        if (p >= n_proteins) return 1;
        ++off[(size_t)p + 1];
    }
    for (uint32_t p = 0; p < n_proteins; ++p) off[(size_t)p + 1] += off[p];
    const uint64_t n_used = off[n_proteins];
    std::vector<uint64_t> next(off.begin(), off.end() - 1);
    std::vector<double> L((size_t)n_used * n);
    for (uint64_t r = 0; r < n_rows; ++r) {  // ascending r: the grouping is stable
        const uint32_t p = protein_of_row[r];
        if (p == maxlfq::NONE) continue;
        const uint64_t g = next[p]++;
        for (uint32_t f = 0; f < n; ++f) L[(size_t)f * n_used + g] = maxlfq::log_of_area(areas[r * n + f]);
    }
    std::vector<double> med(P), A((size_t)n * (n + 1)), fac(n), col(n);
    std::vector<uint32_t> cnt(P), ncol(n);
    std::vector<uint64_t> keys;
    const maxlfq::SerialTeam team;
    for (uint32_t p = 0; p < n_proteins; ++p) {
        const uint64_t a = off[p];
        const uint32_t nr = (uint32_t)(off[(size_t)p + 1] - a);
        uint64_t q = 0;
        for (uint32_t j = 0; j < n; ++j)
            for (uint32_t k = j + 1; k < n; ++k, ++q) {
                if (q != maxlfq::pair_index(j, k, n)) return 1;
                keys.clear();
                for (uint32_t r = 0; r < nr; ++r) {
                    const double x = L[(size_t)j * n_used + a + r], y = L[(size_t)k * n_used + a + r];
                    if (maxlfq::present(x) && maxlfq::present(y)) keys.push_back(maxlfq::key_of(x - y));
                }
                const uint32_t c = (uint32_t)keys.size();
                cnt[q] = c;
                med[q] = maxlfq::missing();
                if (c < mc) continue;
                auto zeros = [&](uint64_t prefix, int bit) {
                    uint32_t z = 0;
                    for (uint64_t key : keys) z += (key >> bit) == (prefix >> bit) ? 1u : 0u;
                    return z;
                };
                uint64_t lo, hi;
                if (c <= 64) {  // (as on the device: few keys are ranked, many selected by radix — any exact selection gives the same bits)
                    std::sort(keys.begin(), keys.end());
                    lo = keys[(c - 1) / 2];
                    hi = keys[c / 2];
                } else {
                    lo = maxlfq::radix_select((c - 1) / 2, zeros);
                    hi = maxlfq::radix_select(c / 2, zeros);
                }
                med[q] = maxlfq::median_of(maxlfq::of_key(lo), maxlfq::of_key(hi), c);
            }
        maxlfq::column_sums(team, L.data() + a, n_used, nr, n, col.data(), ncol.data());
        const uint64_t o = (uint64_t)p * n;
        const maxlfq::Protein v{n, mc, med.data(), cnt.data(), col.data(), ncol.data(), A.data(), fac.data(),
                                log_abundance + o, intensity + o, component + o};
        if (maxlfq::solve(team, v, n_components + p)) return 2 + (int)p;
        n_rows_used[p] = nr;
        if (pair_median && P) std::memcpy(pair_median + (uint64_t)p * P, med.data(), P * 8);
        if (pair_count && P) std::memcpy(pair_count + (uint64_t)p * P, cnt.data(), P * 4);
    }
    return 0;
}

#ifdef MAXLFQ_EMU_MAIN
int main(int argc, char** argv) {
    int worlds = 0;
    for (int i = 1; i < argc; ++i) {
        FILE* fh = std::fopen(argv[i], "rb");
        if (!fh) {
            std::printf("FAILED: cannot open %s\n", argv[i]);
            return 1;
        }
        uint64_t n_rows = 0;
        uint32_t head[4] = {0, 0, 0, 0};
        bool ok = std::fread(&n_rows, 8, 1, fh) == 1 && std::fread(head, 4, 4, fh) == 4;
        const uint32_t n = head[0], np = head[1], mc = head[2];
        std::vector<double> areas(ok ? (size_t)n_rows * n : 0);
        std::vector<uint32_t> protein(ok ? (size_t)n_rows : 0);
        ok = ok && std::fread(areas.data(), 8, areas.size(), fh) == areas.size() &&
             std::fread(protein.data(), 4, protein.size(), fh) == protein.size();
        std::fclose(fh);
        if (!ok) {
            std::printf("FAILED: %s is cut short\n", argv[i]);
            return 1;
        }
        const uint64_t P = maxlfq::n_pairs(n);
        std::vector<double> la((size_t)np * n), inten((size_t)np * n), med((size_t)np * P);
        std::vector<uint32_t> comp((size_t)np * n), used(np), ncomp(np), cnt((size_t)np * P);
        // once with the pair tables, once without: the results must not depend on them
        const int rc = emu_protein_lfq(n_rows, n, np, mc, areas.data(), protein.data(), la.data(), inten.data(), comp.data(), used.data(),
                                       ncomp.data(), med.data(), cnt.data());
        std::vector<double> la2((size_t)np * n), inten2((size_t)np * n);
        std::vector<uint32_t> comp2((size_t)np * n), used2(np), ncomp2(np);
        const int rc2 = emu_protein_lfq(n_rows, n, np, mc, areas.data(), protein.data(), la2.data(), inten2.data(), comp2.data(),
                                        used2.data(), ncomp2.data(), nullptr, nullptr);
        if (rc || rc2 || (!la.empty() && (std::memcmp(la.data(), la2.data(), la.size() * 8) ||
                                          std::memcmp(comp.data(), comp2.data(), comp.size() * 4)))) {
            std::printf("FAILED: %s: status %d / %d, or results that depend on the pair tables\n", argv[i], rc, rc2);
            return 1;
        }
        ++worlds;
    }
    std::printf("maxlfq_emu ok (%d worlds)\n", worlds);
    return 0;
}
#endif
