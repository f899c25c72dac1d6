// Host build of the flat bitmap filter's bookkeeping (sage_amd/csrc/core.h: flat_octets, flat_item_k, flat_item_base / flat_item_ion,
// flat_stride, flat_area_bytes, flat_mask_word) — one wavefront's chunk replayed lane by lane the way kernels.hip: score_candidates runs it — behind a tiny C ABI
// for tests/test_flat_filter_emulation.py.  TEST INFRASTRUCTURE.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../sage_amd/csrc/core.h"

using namespace sagecore;

namespace {
uint32_t bit_of(const uint32_t* bitmap, uint32_t bin) { return (bitmap[(bin & (PBM_BITS - 1u)) >> 5] >> (bin & 31u)) & 1u; }
}  // namespace

extern "C" {

uint32_t emu_flat_octets(uint32_t n_here) { return flat_octets(n_here); }
uint32_t emu_flat_area_bytes(uint32_t total, uint32_t ncharges) { return flat_area_bytes(total, ncharges); }
uint32_t emu_flat_route_wins(uint32_t total, uint32_t longest) { return flat_route_wins(total, longest) ? 1u : 0u; }
uint32_t emu_pbm_words() { return PBM_WORDS; }

// The item list of one chunk: counts[64] octets per lane.  owner[t] / k[t] of every item t as the workers find them (the owner's
// byte in the area, the owner's start from its lane); returns the number of items, or 0xFFFFFFFF if an item's k is not below its
// owner's count.
uint32_t emu_flat_items(const uint32_t* counts, uint32_t* owner, uint32_t* k) {
    uint32_t start[64], total = 0;
    for (uint32_t lane = 0; lane < 64; lane++) { start[lane] = total; total += counts[lane]; }
    std::vector<uint8_t> area(flat_area_bytes(total, 1), 0xEE);
    for (uint32_t lane = 0; lane < 64; lane++)
        for (uint32_t i = 0; i < 8u; i++)
            if (i < counts[lane]) area[start[lane] + i] = (uint8_t)lane;
    for (uint32_t base = 0; base < total; base += 64)
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t t = base + lane;
            if (t >= total) continue;
            owner[t] = area[t];
            k[t] = flat_item_k(t, start[owner[t]]);
            if (k[t] >= counts[owner[t]]) return 0xFFFFFFFFu;
            // the kernel's folded form of the same place, for table offsets below and above 8 start (the base wraps modulo 2^64)
            for (uint64_t at : {(uint64_t)0, (uint64_t)64, (uint64_t)72 * owner[t], (uint64_t)1 << 33})
                if (flat_item_ion(flat_item_base(at, start[owner[t]]), t) != at + 8u * k[t]) return 0xFFFFFFFEu;
        }
    return total;
}

// The chunk at ion j0 of 64 candidates: lane i has nions[i] ions (0: no candidate) in a table of `tstride` floats (its ions, padded
// by 8) — the tables in REVERSE lane order, at ions + tstride (63 - i), so that the last lanes, whose starts are the largest, have the
// smallest table offsets and the folded base wraps — and nfz[i] fragment charges; any_fz2 / any_fz3 as the kernel's ballots (over the
// whole candidates, not the chunk).  m_flat[3 * 64]: the masks by the flat route (the owners' bytes, the workers' octets, the
// three-word read-back); m_lane[3 * 64]: by the per-lane filter's formula (four ions per trip, cut to the chunk).  Returns the number
// of flat trips.
uint32_t emu_flat_masks(const float* ions, uint32_t tstride, uint32_t j0, const uint32_t* nions, const uint32_t* nfz, const uint32_t* bitmap,
                        uint64_t* m_flat, uint64_t* m_lane) {
    bool any_fz2 = false, any_fz3 = false;
    uint32_t n_here[64];
    for (uint32_t i = 0; i < 64; i++) {
        if (nions[i] && nfz[i] >= 2) any_fz2 = true;
        if (nions[i] && nfz[i] >= 3) any_fz3 = true;
        n_here[i] = j0 >= nions[i] ? 0u : nions[i] - j0 < 64u ? nions[i] - j0 : 64u;
    }
    // ---- the per-lane filter (score_candidates' loop, restated)
    for (uint32_t i = 0; i < 64; i++) {
        uint64_t m1 = 0, m2 = 0, m3 = 0;
        if (n_here[i]) {
            const float* q = ions + tstride * (63u - i) + j0;
            for (uint32_t r = 0; r < n_here[i]; r += 4)
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t x = pbm_index(q[r + j]);
                    m1 |= (uint64_t)bit_of(bitmap, pbm_bin_c1(x)) << (r + j);
                    if (any_fz2) m2 |= (uint64_t)bit_of(bitmap, pbm_bin_c2(x)) << (r + j);
                    if (any_fz3) m3 |= (uint64_t)bit_of(bitmap, pbm_bin_c3(x)) << (r + j);
                }
            const uint64_t in_chunk = n_here[i] >= 64u ? ~0ull : (1ull << n_here[i]) - 1ull;
            m1 &= in_chunk;
            m2 = nfz[i] >= 2 ? m2 & in_chunk : 0ull;
            m3 = nfz[i] >= 3 ? m3 & in_chunk : 0ull;
            if (nfz[i] > 3) m1 = m2 = m3 = in_chunk;
        }
        m_lane[i] = m1; m_lane[64 + i] = m2; m_lane[128 + i] = m3;
    }
    // ---- the flat route
    uint32_t cnt[64], start[64], total = 0;
    for (uint32_t i = 0; i < 64; i++) {
        cnt[i] = n_here[i] && nfz[i] <= 3u ? flat_octets(n_here[i]) : 0u;
        start[i] = total;
        total += cnt[i];
    }
    const uint32_t nch = 1u + (any_fz2 ? 1u : 0u) + (any_fz3 ? 1u : 0u), stride = flat_stride(total);
    std::vector<uint8_t> area(flat_area_bytes(total, nch) + 4, 0xEE);  // (+ 4: a read past the area would show as 0xEE bits)
    uint8_t* const a1 = area.data();
    uint8_t* const a2 = a1 + stride;
    uint8_t* const a3 = a2 + (any_fz2 ? stride : 0u);
    for (uint32_t i = 0; i < 64; i++)
        for (uint32_t j = 0; j < 8u; j++)
            if (j < cnt[i]) a1[start[i] + j] = (uint8_t)i;
    uint32_t trips = 0;
    for (uint32_t base = 0; base < total; base += 64, trips++)
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t t = base + lane;
            if (t >= total) continue;
            const uint32_t own = a1[t];
            // (the owner's offer, as it comes through the crossbar, and the worker's place in it)
            const uint64_t ion_at = flat_item_base((uint64_t)tstride * (63u - own) + j0, start[own]);
            const float* q = ions + flat_item_ion(ion_at, t);
            uint32_t b1 = 0, b2 = 0, b3 = 0;
            for (uint32_t j = 0; j < 8; j++) {
                const uint32_t x = pbm_index(q[j]);
                b1 |= bit_of(bitmap, pbm_bin_c1(x)) << j;
                b2 |= bit_of(bitmap, pbm_bin_c2(x)) << j;
                b3 |= bit_of(bitmap, pbm_bin_c3(x)) << j;
            }
            a1[t] = (uint8_t)b1;
            if (any_fz2) a2[t] = (uint8_t)b2;
            if (any_fz3) a3[t] = (uint8_t)b3;
        }
    for (uint32_t i = 0; i < 64; i++) {
        uint64_t m1 = 0, m2 = 0, m3 = 0;
        auto read = [&](const uint8_t* a) {
            uint32_t w[3];
            std::memcpy(w, a + (start[i] & ~3u), 12);
            return (uint64_t)flat_mask_word(w[0], w[1], start[i]) | ((uint64_t)flat_mask_word(w[1], w[2], start[i]) << 32);
        };
        if (cnt[i]) {
            m1 = read(a1);
            if (any_fz2 && nfz[i] >= 2) m2 = read(a2);
            if (any_fz3 && nfz[i] >= 3) m3 = read(a3);
        }
        if (n_here[i]) {
            const uint64_t in_chunk = n_here[i] >= 64u ? ~0ull : (1ull << n_here[i]) - 1ull;
            m1 &= in_chunk;
            m2 = nfz[i] >= 2 ? m2 & in_chunk : 0ull;
            m3 = nfz[i] >= 3 ? m3 & in_chunk : 0ull;
            if (nfz[i] > 3) m1 = m2 = m3 = in_chunk;
        }
        m_flat[i] = m1; m_flat[64 + i] = m2; m_flat[128 + i] = m3;
    }
    return trips;
}

}  // extern "C"
