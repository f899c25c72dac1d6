// Host build of sage_amd/csrc/cover.h — the round logic of the protein-group set cover that the HIP kernels share with the host —
// driven the way the device drives it: every trim step over ALL live edges before the next step begins, the argmax as a
// reduction of CoverKey.  Behind a C ABI for tests/test_protein_groups_cpu.py, and with COVER_EMU_MAIN a stand-alone program
// (a fixed graph family, sanitizer builds).  TEST INFRASTRUCTURE.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sage_amd/csrc/cover.h"

using namespace sagecover;

// cover[n_left] out; returns the number of add_largest picks, or -1 when a loop bound was exceeded.  `reversed` visits the edges
// of every step back to front: the result must not depend on it.
extern "C" int emu_cover(const uint32_t* el, const uint32_t* er, uint32_t n_edges, uint32_t n_left, uint32_t n_right, int reversed,
                         uint8_t* cover) {
    std::vector<uint32_t> ldeg(n_left, 0), rdeg(n_right, 0), lcov(n_left, 0), rcov(n_right, 0);
    for (uint32_t e = 0; e < n_edges; ++e) {
        ldeg[el[e]]++;
        rdeg[er[e]]++;
    }
    const std::vector<uint32_t> odeg(ldeg);
    const Graph g{ldeg.data(), rdeg.data(), lcov.data(), rcov.data(), odeg.data()};
    std::vector<uint8_t> live(n_edges, 1);
    std::vector<uint32_t> order(n_edges);
    for (uint32_t e = 0; e < n_edges; ++e) order[e] = reversed ? n_edges - 1 - e : e;
    uint32_t remaining = n_edges;
    int picks = 0;
    for (uint64_t round = 0; remaining != 0; ++round) {
        if (round > n_edges) return -1;
        for (uint64_t repeat = 0;; ++repeat) {
            if (repeat > n_edges) return -1;
            const uint32_t prev = remaining;
            for (uint32_t e : order)
                if (live[e]) trim_force<PlainAccess>(g, el[e], er[e]);
            for (uint32_t e : order)
                if (live[e] && trim_left<PlainAccess>(g, el[e], er[e])) {
                    live[e] = 0;
                    --remaining;
                }
            for (uint32_t e : order)
                if (live[e] && trim_right<PlainAccess>(g, el[e], er[e])) {
                    live[e] = 0;
                    --remaining;
                }
            if (remaining == prev) break;
        }
        if (remaining == 0) break;
        CoverKey k = key_none();
        if (reversed) {
            for (uint32_t l = n_left; l-- > 0;) k = key_max(k, key_of<PlainAccess>(g, l));
        } else {
            for (uint32_t l = 0; l < n_left; ++l) k = key_max(k, key_of<PlainAccess>(g, l));
        }
        if (k.valid) lcov[k.index] = 1;
        ++picks;
    }
    for (uint32_t l = 0; l < n_left; ++l) cover[l] = (uint8_t)lcov[l];
    return picks;
}

#ifdef COVER_EMU_MAIN
// rings of 3..40 left nodes (every right node shared by two neighbours: no unique evidence, every pick is a tie) next to a chain
// with unique ends; forwards and backwards must agree
int main() {
    for (uint32_t size = 3; size <= 40; ++size) {
        std::vector<uint32_t> el, er;
        for (uint32_t k = 0; k < size; ++k) {
            el.push_back(k);
            er.push_back(k);
            el.push_back((k + 1) % size);
            er.push_back(k);
        }
        for (uint32_t k = 0; k < 5; ++k) {  // a chain: left size + k owns right size + k and size + k + 1
            el.push_back(size + k);
            er.push_back(size + k);
            el.push_back(size + k);
            er.push_back(size + k + 1);
        }
        const uint32_t n_left = size + 5, n_right = size + 6;
        std::vector<uint8_t> a(n_left), b(n_left);
        const int pa = emu_cover(el.data(), er.data(), (uint32_t)el.size(), n_left, n_right, 0, a.data());
        const int pb = emu_cover(el.data(), er.data(), (uint32_t)el.size(), n_left, n_right, 1, b.data());
        if (pa < 1 || pa != pb || a != b) {
            std::printf("ring of %u: %d / %d picks, covers %s\n", size, pa, pb, a == b ? "equal" : "differ");
            return 1;
        }
    }
    std::printf("cover_emu ok\n");
    return 0;
}
#endif
