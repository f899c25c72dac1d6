// Host build of the two-kind forms of the kind walks (sage_amd/csrc/core.h: kinds2_bound / kinds2_nt_mask / kinds2_idx0_c /
// kinds2_decode) — what the KINDS2 instances of kernels.hip: score_candidates use for a table of two ion kinds, kind 0 n-terminal —
// held to the general forms they replace: the kind_seg_first / kind_seg_next walk of a chunk's segments and the
// `while (idx >= lm1)` decode of every ion.  Behind a tiny C ABI for tests/test_two_kinds_emulation.py.
// TEST INFRASTRUCTURE.
#include <cstdint>

#include "../../sage_amd/csrc/core.h"

using namespace sagecore;

extern "C" {

// Every 64-ion chunk (j0 = 0, 64, ... below 2 * lm1) of a candidate with lm1 ions per kind.  Returns the ions checked (2 * lm1), or 0
// with bad[0..2] = {j0, bit, what}.
uint64_t emu_two_kinds(uint32_t lm1, uint64_t* bad) {
    const uint32_t nions = 2u * lm1;
    const uint32_t nterm_mask = 1u;  // (kind 0 is n-terminal, kind 1 is not: what the general form reads from the kind list)
    uint64_t checked = 0;
#define EMU_FAIL(BIT, WHAT) { bad[0] = j0; bad[1] = (BIT); bad[2] = (WHAT); return 0; }
    for (uint32_t j0 = 0; j0 < nions; j0 += 64) {
        const uint32_t n_here = nions - j0 < 64u ? nions - j0 : 64u;
        const uint64_t in_chunk = n_here >= 64u ? ~0ull : (1ull << n_here) - 1ull;
        const uint32_t bound = kinds2_bound(j0, lm1);
        const uint64_t NT = kinds2_nt_mask(bound);
        if (bound > 64u) EMU_FAIL(0, 1)
        // the boundary is lm1 - j0 clamped to [0, 64]
        const int64_t raw = (int64_t)lm1 - (int64_t)j0;
        if (bound != (uint32_t)(raw < 0 ? 0 : raw > 64 ? 64 : raw)) EMU_FAIL(0, 2)
        // ---- the general walk's segments: NT mask (the one-trip route's loop) and (mask, shift, idx0) per kind (counts and runs)
        uint64_t NT_walk = 0, seg_mask[2] = {0, 0};
        uint32_t seg_lo[2] = {0, 0}, seg_idx0[2] = {0, 0}, segs = 0;
        for (KindSeg g = kind_seg_first(j0, lm1); g.lo < n_here; g = kind_seg_next(g, lm1)) {
            if (g.kind > 1u) EMU_FAIL(g.lo, 3)
            const uint64_t seg = kind_seg_mask(g);
            if ((nterm_mask >> g.kind) & 1u) NT_walk |= seg;
            if (seg_mask[g.kind]) EMU_FAIL(g.lo, 4)  // (one segment per kind and chunk)
            seg_mask[g.kind] = seg & in_chunk;
            seg_lo[g.kind] = g.lo;
            seg_idx0[g.kind] = g.idx0;
            segs++;
        }
        if (segs == 0u || segs > 2u) EMU_FAIL(0, 5)
        if ((NT_walk & in_chunk) != (NT & in_chunk)) EMU_FAIL(0, 6)
        // kind 0: the bits below the boundary, index j0 at bit 0 (what run_matched_mask is handed: K & NT, idx0 = j0)
        if (seg_mask[0] != (NT & in_chunk)) EMU_FAIL(0, 7)
        if (seg_mask[0] && (seg_lo[0] != 0u || seg_idx0[0] != j0)) EMU_FAIL(0, 8)
        // kind 1: every bit from the boundary on (K & ~NT, shifted down by the boundary), its first index kinds2_idx0_c
        if (seg_mask[1] != (~NT & in_chunk)) EMU_FAIL(0, 9)
        if (seg_mask[1] && (bound >= 64u || seg_lo[1] != bound || seg_idx0[1] != kinds2_idx0_c(j0, lm1))) EMU_FAIL(0, 10)
        // ---- every ion: the subtract loop's (kind, index) against the decode and against the mask
        for (uint32_t t = 0; t < n_here; t++) {
            uint32_t kind = 0, idx = j0 + t;
            while (idx >= lm1) { idx -= lm1; kind++; }
            bool cterm = false;
            const uint32_t idx2 = kinds2_decode(j0 + t, lm1, cterm);
            if (kind > 1u || (kind == 1u) != cterm || idx != idx2) EMU_FAIL(t, 11)
            if ((((nterm_mask >> kind) & 1u) != 0u) != !cterm) EMU_FAIL(t, 12)
            if ((((NT >> t) & 1ull) != 0ull) != !cterm) EMU_FAIL(t, 13)
            // (the index run_matched_mask works out for bit t of its shifted mask)
            const uint32_t via_mask = cterm ? kinds2_idx0_c(j0, lm1) + (t - bound) : j0 + t;
            if (via_mask != idx) EMU_FAIL(t, 14)
            checked++;
        }
    }
#undef EMU_FAIL
    return checked;
}

// The cooperative path's counts and runs for one chunk, both ways: hit masks K1 / K2 / K3 (bits inside the candidate's ions) into the
// packed match counts and the two Run states.  out[0..2] = {mm, b_run, y_run} of the general walk, out[3..5] of the two-kind form.
void emu_two_kinds_counts(uint32_t lm1, uint32_t j0, uint64_t K1, uint64_t K2, uint64_t K3, uint32_t mm, uint32_t b_run, uint32_t y_run,
                          uint32_t* out) {
    const uint32_t nterm_mask = 1u;
    {
        uint32_t u_mm = mm, u_b = b_run, u_y = y_run;
        uint64_t anyK = K1 | K2 | K3;
        for (KindSeg g = kind_seg_first(j0, lm1); anyK && g.lo < 64u; g = kind_seg_next(g, lm1)) {
            const uint64_t seg = kind_seg_mask(g);
            const uint64_t S = anyK & seg;
            if (!S) continue;
            anyK ^= S;
            const bool nterm = (nterm_mask >> g.kind) & 1u;
            u_mm += (uint32_t)(__builtin_popcountll(K1 & seg) + __builtin_popcountll(K2 & seg) + __builtin_popcountll(K3 & seg)) << (nterm ? 0u : 16u);
            if (nterm) run_matched_mask(u_b, S >> g.lo, g.idx0);
            else run_matched_mask(u_y, S >> g.lo, g.idx0);
        }
        out[0] = u_mm; out[1] = u_b; out[2] = u_y;
    }
    {
        uint32_t u_mm = mm, u_b = b_run, u_y = y_run;
        const uint64_t anyK = K1 | K2 | K3;
        const uint32_t bound = kinds2_bound(j0, lm1);
        const uint64_t NT = kinds2_nt_mask(bound);
        const uint64_t Sb = anyK & NT, Sy = anyK & ~NT;
        if (Sb) {
            u_mm += (uint32_t)(__builtin_popcountll(K1 & NT) + __builtin_popcountll(K2 & NT) + __builtin_popcountll(K3 & NT));
            run_matched_mask(u_b, Sb, j0);
        }
        if (Sy) {
            u_mm += (uint32_t)(__builtin_popcountll(K1 & ~NT) + __builtin_popcountll(K2 & ~NT) + __builtin_popcountll(K3 & ~NT)) << 16;
            run_matched_mask(u_y, Sy >> bound, kinds2_idx0_c(j0, lm1));
        }
        out[3] = u_mm; out[4] = u_b; out[5] = u_y;
    }
}

}  // extern "C"
