// Host build of the item order of a heavy candidate's chunk (sage_amd/csrc/core.h: coop_items_below, coop_item_pos) — where the
// one-trip route of kernels.hip: score_candidates puts every (ion, fragment charge) item of the chunk, one per lane — held to the
// plain enumeration it stands for: ion by ion, charge by charge, counting.  And the route's three sums as the kernel makes them —
// a slot per item, +0.0f where the item adds nothing to that sum and from the last item on, every slot added, four at a time —
// held bit for bit to the reference's additions of the matched items alone.  A stand-alone program (its own main, no Python):
// tests/test_coop_items_emulation.py runs it; it can be built with the host sanitizers as it is.
//
//     coop_items_emu exhaustive            every triple of masks over 6 bits (at every shift that keeps it inside 64 bits: 0, 29, 58)
//     coop_items_emu random SEED COUNT     random 64-bit triples of every density, the empty and the full ones among them
//     coop_items_emu edges                 empty masks, a full M1 (N = 64), N = 65, bit 63
//     coop_items_emu segments              lm1 1 .. 70 x 1 .. 8 kinds x every chunk: the kind segments' item ranges
//     coop_items_emu sums SEED COUNT       the slot sums against the sequential sums, signed zeros and denormals among the values
//
// Prints "ok <cases>" and returns 0, or the first case that differs and returns 1.  TEST INFRASTRUCTURE.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../sage_amd/csrc/core.h"

using namespace sagecore;

namespace {
struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint64_t mask(uint32_t density) {  // density 0 .. 4: empty, sparse, half, dense, full
        switch (density) {
            case 0: return 0ull;
            case 1: return next() & next() & next();
            case 2: return next();
            case 3: return next() | next() | next();
            default: return ~0ull;
        }
    }
};

// the plain enumeration: position of every item, -1 where the ion has none at that charge; returns N
uint32_t enumerate(const uint64_t M[3], int pos[64][3]) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < 64; i++)
        for (uint32_t c = 0; c < 3; c++) pos[i][c] = ((M[c] >> i) & 1ull) ? (int)n++ : -1;
    return n;
}

bool check_triple(const uint64_t M[3]) {
    int pos[64][3];
    const uint32_t n = enumerate(M, pos);
    uint32_t below = 0;
    for (uint32_t i = 0; i <= 64; i++) {
        if (coop_items_below(M[0], M[1], M[2], i) != below) {
            printf("BAD coop_items_below(%#" PRIx64 ", %#" PRIx64 ", %#" PRIx64 ", %u) = %u, enumeration %u\n", M[0], M[1], M[2], i,
                   coop_items_below(M[0], M[1], M[2], i), below);
            return false;
        }
        if (i == 64) break;
        for (uint32_t c = 0; c < 3; c++) {
            if (pos[i][c] < 0) continue;
            below++;
            if (coop_item_pos(M[0], M[1], M[2], i, c + 1) != (uint32_t)pos[i][c]) {
                printf("BAD coop_item_pos(%#" PRIx64 ", %#" PRIx64 ", %#" PRIx64 ", ion %u, charge %u) = %u, enumeration %d\n", M[0], M[1], M[2], i,
                       c + 1, coop_item_pos(M[0], M[1], M[2], i, c + 1), pos[i][c]);
                return false;
            }
        }
    }
    // (N, which decides the route: <= COOP_ITEMS_CAP takes it)
    if (below != n || coop_items_below(M[0], M[1], M[2], 64) != n) {
        printf("BAD N of %#" PRIx64 ", %#" PRIx64 ", %#" PRIx64 "\n", M[0], M[1], M[2]);
        return false;
    }
    return true;
}

int exhaustive() {
    uint64_t cases = 0;
    for (uint32_t shift : {0u, 29u, 58u})
        for (uint64_t a = 0; a < 64; a++)
            for (uint64_t b = 0; b < 64; b++)
                for (uint64_t c = 0; c < 64; c++) {
                    const uint64_t M[3] = {a << shift, b << shift, c << shift};
                    if (!check_triple(M)) return 1;
                    cases++;
                }
    printf("ok %" PRIu64 "\n", cases);
    return 0;
}

int random_triples(uint64_t seed, uint64_t count) {
    Rng rng{seed};
    for (uint64_t k = 0; k < count; k++) {
        const uint64_t d = rng.next();
        const uint64_t M[3] = {rng.mask((uint32_t)(d % 5)), rng.mask((uint32_t)((d >> 8) % 5)), rng.mask((uint32_t)((d >> 16) % 5))};
        if (!check_triple(M)) return 1;
    }
    printf("ok %" PRIu64 "\n", count);
    return 0;
}

int edges() {
    const uint64_t sets[][3] = {
        {0ull, 0ull, 0ull},                                    // nothing: N = 0
        {~0ull, 0ull, 0ull},                                   // a full M1: N = 64, the last chunk the route takes
        {~0ull, 1ull, 0ull},       {~0ull, 0ull, 1ull << 63},  // N = 65: the route falls back
        {~0ull, ~0ull, ~0ull},                                 // N = 192
        {1ull << 63, 1ull << 63, 1ull << 63},                  // the last ion at all three charges
        {0ull, ~0ull, 0ull},       {0ull, 0ull, ~0ull},        // a charge without the ones below it
        {0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull, 0ull},  // N = 64 over two charges
    };
    const uint32_t want_n[] = {0, 64, 65, 65, 192, 3, 64, 64, 64};
    uint64_t cases = 0;
    for (const auto& M : sets) {
        if (!check_triple(M)) return 1;
        const uint32_t n = coop_items_below(M[0], M[1], M[2], 64);
        if (n != want_n[cases] || (n <= COOP_ITEMS_CAP) != (want_n[cases] <= 64u)) {
            printf("BAD N = %u of edge case %" PRIu64 ", expected %u\n", n, cases, want_n[cases]);
            return 1;
        }
        cases++;
    }
    printf("ok %" PRIu64 "\n", cases);
    return 0;
}

// a kind segment's items are the positions [coop_items_below(lo), coop_items_below(lo + len)): every item of an ion whose kind —
// by the subtract loop — is the segment's lies inside, every other outside, for all chunks of a table of lm1 ions x n_kinds kinds
int segments() {
    Rng rng{71};
    uint64_t cases = 0;
    for (uint32_t lm1 = 1; lm1 <= 70; lm1++)
        for (uint32_t n_kinds = 1; n_kinds <= 8; n_kinds++) {
            const uint32_t nions = lm1 * n_kinds;
            for (uint32_t j0 = 0; j0 < nions; j0 += 64) {
                const uint32_t n_here = nions - j0 < 64u ? nions - j0 : 64u;
                const uint64_t in_chunk = n_here >= 64u ? ~0ull : (1ull << n_here) - 1ull;
                const uint64_t M[3] = {rng.next() & in_chunk, rng.next() & rng.next() & in_chunk, rng.next() & rng.next() & in_chunk};
                int pos[64][3];
                enumerate(M, pos);
                uint32_t covered = 0;
                for (KindSeg g = kind_seg_first(j0, lm1); g.lo < n_here; g = kind_seg_next(g, lm1)) {
                    const uint32_t first = coop_items_below(M[0], M[1], M[2], g.lo), end = coop_items_below(M[0], M[1], M[2], g.lo + g.len);
                    if (first != covered) { printf("BAD segment start: lm1 %u kinds %u j0 %u lo %u\n", lm1, n_kinds, j0, g.lo); return 1; }
                    covered = end;
                    for (uint32_t i = 0; i < n_here; i++) {
                        uint32_t kind = 0, idx = j0 + i;
                        while (idx >= lm1) { idx -= lm1; kind++; }
                        for (uint32_t c = 0; c < 3; c++) {
                            if (pos[i][c] < 0) continue;
                            const bool inside = (uint32_t)pos[i][c] >= first && (uint32_t)pos[i][c] < end;
                            if (inside != (kind == g.kind)) {
                                printf("BAD segment range: lm1 %u kinds %u j0 %u ion %u charge %u kind %u, segment kind %u [%u, %u)\n", lm1, n_kinds,
                                       j0, i, c + 1, kind, g.kind, first, end);
                                return 1;
                            }
                        }
                    }
                }
                if (covered != coop_items_below(M[0], M[1], M[2], 64)) { printf("BAD cover: lm1 %u kinds %u j0 %u\n", lm1, n_kinds, j0); return 1; }
                cases++;
            }
        }
    printf("ok %" PRIu64 "\n", cases);
    return 0;
}

uint32_t bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
float float_of(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// The sums.  Reference: start at the candidate's sums so far (which began at +0.0f: never -0.0f), add every matched item in item
// order — its intensity to the n-terminal or the other sum, its ppm term to the third.  Route: three arrays of 64 slots, +0.0f
// wherever an item adds nothing, every slot of the first ceil(N / 4) fours added in order.
int sums(uint64_t seed, uint64_t count) {
    Rng rng{seed};
    const float specials[] = {0.0f, -0.0f, float_of(1u), float_of(0x80000001u), 1e-30f, -1e-30f, 3.0e38f, -3.0e38f, 1.0f, 16777216.0f};
    auto value = [&]() {
        const uint64_t r = rng.next();
        if (r % 4 == 0) return specials[(r >> 8) % (sizeof(specials) / sizeof(specials[0]))];
        return (float)((double)((r >> 11) % 2000001) * 0.37 - ((r >> 40) % 3 == 0 ? 370000.0 : 0.0));
    };
    for (uint64_t k = 0; k < count; k++) {
        const uint32_t n = (uint32_t)(rng.next() % 65);
        // sums so far: from +0.0f through earlier additions (so possibly +0.0f itself, never -0.0f)
        float start[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t a = 0; a < 3; a++)
            for (uint32_t t = (uint32_t)(rng.next() % 3); t; t--) start[a] += value();
        float ref[3] = {start[0], start[1], start[2]};
        float slot[3][64];
        for (uint32_t p = 0; p < 64; p++) slot[0][p] = slot[1][p] = slot[2][p] = 0.0f;
        for (uint32_t p = 0; p < n; p++) {
            const uint64_t r = rng.next();
            const bool matched = (r & 3u) != 0u, nterm = (r >> 2) & 1u;
            if (!matched) continue;
            const float it = value(), tm = value();
            ref[nterm ? 0 : 1] += it;
            ref[2] += tm;
            slot[nterm ? 0 : 1][p] = it;
            slot[2][p] = tm;
        }
        for (uint32_t a = 0; a < 3; a++) {
            float acc = start[a];
            for (uint32_t q = 0; q == 0 || q < n; q += 4) {
                acc += slot[a][q];
                acc += slot[a][q + 1];
                acc += slot[a][q + 2];
                acc += slot[a][q + 3];
            }
            if (bits_of(acc) != bits_of(ref[a]) && !(acc != acc && ref[a] != ref[a])) {
                printf("BAD sum %u of case %" PRIu64 " (N = %u): slots %#x, sequential %#x\n", a, k, n, bits_of(acc), bits_of(ref[a]));
                return 1;
            }
        }
    }
    printf("ok %" PRIu64 "\n", count);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    const char* what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "exhaustive")) return exhaustive();
    if (!strcmp(what, "random") && argc == 4) return random_triples(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    if (!strcmp(what, "edges")) return edges();
    if (!strcmp(what, "segments")) return segments();
    if (!strcmp(what, "sums") && argc == 4) return sums(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    fprintf(stderr, "usage: coop_items_emu exhaustive | random SEED COUNT | edges | segments | sums SEED COUNT\n");
    return 2;
}
