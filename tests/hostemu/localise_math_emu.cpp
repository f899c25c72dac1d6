// localise_math_emu.cpp — the f64 arithmetic of site localisation (sage_amd/csrc/localise_math.h) as a program of its own, built
// with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_localise_cpu.py.  What no call through the library reaches:
// DepthScores starts its cache again once it holds more than 2^23 values, and a value must not depend on whether it was computed
// before that, after it, or by a cache that never filled.
#include <cstdio>
#include <cstring>

#include "../../sage_amd/csrc/localise_math.h"

namespace {

struct Key {
    uint32_t n, N, d;
};
const Key KEYS[] = {{1, 1, 10}, {3, 10, 4}, {17, 300, 7}, {600, 600, 1}, {1, 65535, 1}, {65000, 65535, 10}, {65535, 65535, 3}, {0, 5, 1}, {2, 0, 9}};
constexpr int N_KEYS = (int)(sizeof KEYS / sizeof KEYS[0]);

uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}

void read_keys(DepthScores& ds, uint64_t* out) {
    for (int k = 0; k < N_KEYS; k++) out[k] = bits(ds.get(KEYS[k].n, KEYS[k].N, KEYS[k].d));
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        failures++;
    }
}

}  // namespace

int main() {
    DepthScores ds;
    uint64_t before[N_KEYS], cached[N_KEYS], after[N_KEYS], fresh[N_KEYS];
    read_keys(ds, before);
    read_keys(ds, cached);
    expect(std::memcmp(before, cached, sizeof before) == 0, "a kept value differs from the computed one");
    expect(before[N_KEYS - 2] == bits(0.0) && before[N_KEYS - 1] == bits(0.0), "n == 0 or N == 0 is not +0.0");

    // a table of 10 * N values per N: 65535, 65534, ... until the cache has started again (13 tables pass 2^23 values, the
    // request after them clears)
    int restarts = 0, tables = 0;
    for (uint32_t N = 65535; N > 65535 - 20 && restarts == 0; N--, tables++) {
        const size_t kept = ds.kept;
        const double v = ds.get(N, N, 1);  // P = 0.01 ^ N: one term
        expect(v > 0.0 && std::isfinite(v), "S(N, N, 1) is not a finite positive score");
        if (ds.kept < kept) restarts++;
    }
    expect(restarts == 1, "the cache did not start again within 20 tables");
    expect(tables >= 13, "the cache started again before it held 2^23 values");
    expect(ds.kept <= (size_t)65535 * 10, "the restarted cache kept old tables");

    read_keys(ds, after);
    expect(std::memcmp(before, after, sizeof before) == 0, "a value computed after the restart differs from the one before it");
    DepthScores other;
    read_keys(other, fresh);
    expect(std::memcmp(before, fresh, sizeof before) == 0, "a fresh cache computes another value");

    // ascore_of: no site-determining items; a tie between depths goes to the smallest
    {
        const uint16_t a[10] = {3, 4, 5, 5, 5, 5, 5, 5, 5, 5}, b[10] = {1, 2, 3, 3, 3, 3, 3, 3, 3, 3};
        uint8_t depth = 77;
        expect(bits(ascore_of(ds, a, b, 0, depth)) == bits(0.0) && depth == 1, "Ns == 0: not (0.0, depth 1)");
        depth = 77;
        const double all_tied = ascore_of(ds, a, b, 6, depth);  // a - b = 2 at every depth
        expect(depth == 1 && bits(all_tied) == bits(other.get(3, 6, 1) - other.get(1, 6, 1)), "a tie of all depths does not go to depth 1");
        const uint16_t a2[10] = {2, 5, 6, 6, 6, 4, 3, 3, 3, 3}, b2[10] = {1, 2, 3, 4, 5, 4, 3, 3, 3, 3};
        depth = 77;
        const double tied = ascore_of(ds, a2, b2, 6, depth);  // a - b = 1 3 3 2 1 0 ...: depths 2 and 3 tie
        expect(depth == 2 && bits(tied) == bits(other.get(5, 6, 2) - other.get(2, 6, 2)), "a tie of depths 2 and 3 does not go to depth 2");
        const uint16_t n[10] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
        double sum = 0.0;
        for (uint32_t d = 1; d <= 10; d++) sum += LOC_WEIGHT[d - 1] * other.get(1, 1, d);
        expect(bits(peptide_score(ds, n, 1)) == bits(sum / 7.0), "peptide_score is not the weighted sum over 7");
    }
    if (failures) return 1;
    std::printf("localise_math_emu ok (%d tables before the restart)\n", tables);
    return 0;
}
