// Host build of the mask forms of Run (sage_amd/csrc/core.h: run_matched_mask, kind_seg_first / kind_seg_next / kind_seg_mask) —
// what the cooperative path of kernels.hip: score_candidates takes a heavy candidate's runs and kind segments from — held to the
// sequential forms they replace: run_matched_packed once (or several times) per set bit in ascending order, and the
// `while (idx >= lm1)` walk that finds an ion's kind and index.  Behind a tiny C ABI for tests/test_run_mask_emulation.py.
// TEST INFRASTRUCTURE.
#include <cstdint>
#include <initializer_list>

#include "../../sage_amd/csrc/core.h"

using namespace sagecore;

namespace {
template <class R> struct Fields;
template <> struct Fields<uint32_t> { static constexpr uint32_t BITS = 10; };
template <> struct Fields<uint64_t> { static constexpr uint32_t BITS = 21; };
template <class R>
R pack(uint32_t next, uint32_t length, uint32_t longest) {
    return (R)next | ((R)length << Fields<R>::BITS) | ((R)longest << (2 * Fields<R>::BITS));
}
// the sequential form: every set bit of S in ascending order, bit t offered 1 + (reps >> 2t & 3) % 3 times
template <class R>
R sequential(R r, uint64_t S, uint32_t idx0, const uint64_t reps[2]) {
    for (uint32_t t = 0; t < 64; t++) {
        if (!((S >> t) & 1ull)) continue;
        const uint32_t n = 1u + (uint32_t)((reps[t >> 5] >> (2u * (t & 31u))) & 3ull) % 3u;
        for (uint32_t k = 0; k < n; k++) run_matched_packed(r, idx0 + t);
    }
    return r;
}
struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};
template <class R>
bool same(R r, uint64_t S, uint32_t idx0, const uint64_t reps[2], uint64_t* bad) {
    R got = r;
    run_matched_mask(got, S, idx0);
    const R want = sequential(r, S, idx0, reps);
    if (got == want) return true;
    if (bad) { bad[0] = (uint64_t)r; bad[1] = S; bad[2] = idx0; bad[3] = (uint64_t)got; bad[4] = (uint64_t)want; }
    return false;
}

// every S below 2^16 x idx0 in {0, 1, 2, 7} x carried states: fresh; next in {idx0 - 1, idx0, idx0 + 1, idx0 + 2, idx0 + 5} where
// non-negative x length in {1, 3} x longest in {length, length + 4}
template <class R>
uint64_t exhaustive(uint64_t* bad) {
    const uint64_t once[2] = {0, 0};
    uint64_t cases = 0;
    for (uint32_t idx0 : {0u, 1u, 2u, 7u}) {
        R states[21];
        uint32_t ns = 0;
        states[ns++] = 0;
        for (int dn : {-1, 0, 1, 2, 5}) {
            if ((int)idx0 + dn < 0) continue;
            for (uint32_t length : {1u, 3u})
                for (uint32_t longest : {length, length + 4u}) states[ns++] = pack<R>(idx0 + (uint32_t)dn, length, longest);
        }
        for (uint32_t si = 0; si < ns; si++)
            for (uint64_t S = 0; S < (1ull << 16); S++) {
                cases++;
                if (!same<R>(states[si], S, idx0, once, bad)) return 0;
            }
    }
    return cases;
}

// 64-bit masks (sparse, dense, full, bit 63 set among them), idx0 up to max_idx0, every bit offered one to three times; the carried
// state is what an earlier mask at an earlier — or, as behind a kind of the same series, a LATER — place left
template <class R>
uint64_t random_masks(uint64_t seed, uint64_t n, uint32_t max_idx0, uint64_t* bad) {
    Rng g{seed};
    const uint64_t once[2] = {0, 0};
    uint64_t with63 = 0, full = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t S = g.next();
        switch (g.next() % 8) {
            case 0: S &= g.next() & g.next(); break;  // sparse
            case 1: S |= g.next() | g.next(); break;  // long runs
            case 2: S = ~0ull; break;
            case 3: S |= 1ull << 63; break;
            case 4: S = ~0ull << (g.next() % 64); break;
            case 5: S = ~0ull >> (g.next() % 64); break;
            default: break;
        }
        with63 += S >> 63;
        full += S == ~0ull;
        const uint32_t idx0 = (uint32_t)(g.next() % (max_idx0 + 1u));
        R r = 0;
        switch (g.next() % 4) {
            case 0: break;  // fresh
            case 1: {       // an earlier chunk of the same kind: ends right in front of idx0, or further back
                const uint32_t back = (uint32_t)(g.next() % 3) ? 64u : 64u + (uint32_t)(g.next() % 64);
                if (idx0 >= back) run_matched_mask(r, g.next() | (g.next() % 2 ? 1ull << 63 : 0ull), idx0 - back);
                break;
            }
            case 2:  // an earlier kind of the same series: anywhere, `last` beyond idx0 included
                run_matched_mask(r, g.next() & g.next(), (uint32_t)(g.next() % (max_idx0 + 1u)));
                run_matched_mask(r, g.next(), (uint32_t)(g.next() % (max_idx0 + 1u)));
                break;
            default: {  // `last` on one of this mask's own bits
                const uint32_t at = idx0 + (uint32_t)(g.next() % 64);
                run_matched_mask(r, g.next() % 2 ? 1ull : 7ull, at >= 2u ? at - (uint32_t)(g.next() % 3) : at);
                break;
            }
        }
        const uint64_t reps[2] = {g.next(), g.next()};
        if (!same<R>(r, S, idx0, reps, bad)) return 0;
        // (and several calls per bit leave what one call leaves)
        if (sequential(r, S, idx0, reps) != sequential(r, S, idx0, once)) return 0;
    }
    return with63 && full ? n : 0;
}
}  // namespace

extern "C" {

uint32_t emu_run_mask32(uint32_t r, uint64_t S, uint32_t idx0) { run_matched_mask(r, S, idx0); return r; }
uint64_t emu_run_mask64(uint64_t r, uint64_t S, uint32_t idx0) { run_matched_mask(r, S, idx0); return r; }
uint32_t emu_run_seq32(uint32_t r, uint64_t S, uint32_t idx0, uint32_t times) {
    const uint64_t reps[2] = {times == 2 ? 0x5555555555555555ull : times == 3 ? 0xAAAAAAAAAAAAAAAAull : 0ull,
                              times == 2 ? 0x5555555555555555ull : times == 3 ? 0xAAAAAAAAAAAAAAAAull : 0ull};
    return sequential(r, S, idx0, reps);
}
uint64_t emu_run_seq64(uint64_t r, uint64_t S, uint32_t idx0, uint32_t times) {
    const uint64_t reps[2] = {times == 2 ? 0x5555555555555555ull : times == 3 ? 0xAAAAAAAAAAAAAAAAull : 0ull,
                              times == 2 ? 0x5555555555555555ull : times == 3 ? 0xAAAAAAAAAAAAAAAAull : 0ull};
    return sequential(r, S, idx0, reps);
}

// cases checked, or 0 with bad[0..4] = {state, S, idx0, mask form, sequential form} of the first case that differs
uint64_t emu_run_mask_exhaustive(uint32_t wide, uint64_t* bad) { return wide ? exhaustive<uint64_t>(bad) : exhaustive<uint32_t>(bad); }
uint64_t emu_run_mask_random(uint32_t wide, uint64_t seed, uint64_t n, uint32_t max_idx0, uint64_t* bad) {
    return wide ? random_masks<uint64_t>(seed, n, max_idx0, bad) : random_masks<uint32_t>(seed, n, max_idx0, bad);
}

// The kind segments of every 64-ion chunk of a candidate with lm1 ions per kind and n_kinds kinds against the walk
// `kind = 0, idx = j; while (idx >= lm1) { idx -= lm1; kind++; }` of every ion j: the segments tile the chunk's ions in order,
// none is empty, one per kind the chunk meets (at most n_kinds, two with lm1 >= 64), and every ion's (kind, index)
// is its segment's (kind, idx0 + its place in the segment).  Returns the ions checked, or 0 with bad[0..2] = {j0, bit, what}.
uint64_t emu_kind_segments(uint32_t lm1, uint32_t n_kinds, uint64_t* bad) {
    const uint32_t nions = lm1 * n_kinds;
    uint64_t checked = 0;
    for (uint32_t j0 = 0; j0 < nions; j0 += 64) {
        const uint32_t n_here = nions - j0 < 64u ? nions - j0 : 64u;
        uint64_t covered = 0;
        uint32_t segs = 0;
        KindSeg g = kind_seg_first(j0, lm1);
        uint32_t expect_lo = 0;
        while (g.lo < n_here) {
            const uint64_t seg = kind_seg_mask(g);
#define EMU_FAIL(WHAT) { bad[0] = j0; bad[1] = g.lo; bad[2] = (WHAT); return 0; }
            if (g.lo != expect_lo || g.len == 0 || g.lo + g.len > 64u || g.idx0 + g.len > lm1) EMU_FAIL(1)
            if (seg & covered) EMU_FAIL(2)
            if (g.lo != 0u && g.idx0 != 0u) EMU_FAIL(3)  // (only a chunk's first segment starts inside a kind)
            for (uint32_t t = g.lo; t < g.lo + g.len && t < n_here; t++) {
                if (!((seg >> t) & 1ull)) EMU_FAIL(4)
                uint32_t kind = 0, idx = j0 + t;
                while (idx >= lm1) { idx -= lm1; kind++; }
                if (kind != g.kind || idx != g.idx0 + (t - g.lo)) EMU_FAIL(5)
                checked++;
            }
            if (g.len < 64u && (seg >> g.lo) != (1ull << g.len) - 1ull) EMU_FAIL(6)
            covered |= seg;
            expect_lo = g.lo + g.len;
            segs++;
            g = kind_seg_next(g, lm1);
        }
        const uint64_t in_chunk = n_here >= 64u ? ~0ull : (1ull << n_here) - 1ull;
        if ((covered & in_chunk) != in_chunk) EMU_FAIL(7)
        if (segs > n_kinds || segs > 64u / lm1 + 2u) EMU_FAIL(8)  // (one segment per kind the chunk meets)
#undef EMU_FAIL
    }
    return checked;
}

}  // extern "C"
