// Host build of sage_amd/csrc/crlog.h's cr_log1pf for tests/test_ln1pf_cpu.py: the function itself, the reference it is held to
// (libquadmath's 113-bit log1pq rounded ONCE to f32) and a sweep over a range of f32 bit patterns that compares the two.
#include <math.h>
#include <quadmath.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../sage_amd/csrc/crlog.h"

namespace {
float from_bits(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
uint32_t bits_of(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
uint64_t bits_of(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
bool same(float a, float b) { return (a != a && b != b) || bits_of(a) == bits_of(b); }  // (any NaN equals any NaN)
float ref_quad(float x) { return (float)log1pq((__float128)x); }
// a float's place on the number line as an integer: the distance of two floats in ulps is the difference of their keys
int64_t order_key(float x) { const uint32_t u = bits_of(x); return (u & 0x80000000u) ? -(int64_t)(u & 0x7FFFFFFFu) : (int64_t)u; }

const uint32_t TINY = 0x2B800000u;   // 2^-40: below it the result is the argument (asserted directly)
const uint32_t FILTER_ULPS = 8;      // glibc's f64 log1p this many f64 ulps or less from a rounding boundary of f32: ask quad
const uint32_t AUDIT_EVERY = 4099;   // ... and ask quad on every 4099th pattern whatever the filter says

// The reference by the filter: glibc's f64 log1p (< 1 ulp) rounded to f32 where it is more than FILTER_ULPS f64 ulps away from
// the midpoint of two floats, libquadmath elsewhere.  Only for normal f32 results (|x| >= 2^-40 here): a subnormal result's
// boundaries are not where the low 29 bits of the double say.
float ref_filtered(float x, bool& hard) {
    const double d = log1p((double)x);
    const uint32_t low = (uint32_t)(bits_of(d) & 0x1FFFFFFFull);
    hard = (low > 0x10000000u ? low - 0x10000000u : 0x10000000u - low) <= FILTER_ULPS;
    return hard ? ref_quad(x) : (float)d;
}

struct Tally {
    uint64_t mismatches = 0, hard = 0, audited = 0, audit_failures = 0, libm_compared = 0, libm_wrong = 0, libm_max_ulp = 0,
             libm_max_ulp_arg = 0;
    std::vector<uint32_t> mism, hards, wrongs;
};

void sweep_range(uint64_t first, uint64_t last, uint32_t cap, Tally& t) {
    for (uint64_t p = first; p < last; p++) {
        const uint32_t u = (uint32_t)p, a = u & 0x7FFFFFFFu;
        const float x = from_bits(u);
        const float got = sagecore::cr_log1pf(x);
        float want;
        bool hard = false;
        const bool finite_domain = a < 0x7F800000u && !(u > 0xBF800000u);  // not inf / NaN, not below -1
        if (a < TINY) {
            want = x;
        } else if (!finite_domain || u == 0xBF800000u) {
            want = x != x || x < -1.0f ? NAN : x == -1.0f ? -INFINITY : x;  // (+inf -> +inf, -inf -> NaN by x < -1)
        } else {
            want = ref_filtered(x, hard);
            if (hard) { t.hard++; if (t.hards.size() < cap) t.hards.push_back(u); }
        }
        if (p % AUDIT_EVERY == 0) {  // the filter's own audit: quad unconditionally
            t.audited++;
            if (!same(want, ref_quad(x))) t.audit_failures++;
        }
        if (!same(got, want)) { t.mismatches++; if (t.mism.size() < cap) t.mism.push_back(u); }
        if (finite_domain && a >= TINY && !(u & 0x80000000u)) {  // census of the platform's log1pf on the positive arguments
            const float m = log1pf(x);
            t.libm_compared++;
            if (!same(m, want)) {
                t.libm_wrong++;
                if (t.wrongs.size() < cap) t.wrongs.push_back(u);
                const int64_t dist = order_key(m) - order_key(want);
                const uint64_t ad = (uint64_t)(dist < 0 ? -dist : dist);
                if (ad > t.libm_max_ulp) { t.libm_max_ulp = ad; t.libm_max_ulp_arg = u; }
            }
        }
    }
}
}  // namespace

extern "C" {
void emu_cr_log1pf(const float* x, uint64_t n, float* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = sagecore::cr_log1pf(x[i]);
}
void emu_ref_ln1pf(const float* x, uint64_t n, float* out) {  // libquadmath, rounded once
    for (uint64_t i = 0; i < n; i++) out[i] = ref_quad(x[i]);
}
void emu_libm_log1pf(const float* x, uint64_t n, float* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = log1pf(x[i]);
}
// Bit patterns [first, last) on `threads` threads.  stats[8]: mismatches of cr_log1pf, hard arguments (quad asked by the filter),
// audited patterns, audit failures, positive arguments on which the platform's log1pf was compared, those it got wrong, its
// largest distance from the reference in f32 ulps, the argument of that distance.  The three lists (each `cap` long, in
// ascending order, the first `cap` of the range): mismatching patterns, hard arguments, arguments the platform's log1pf gets wrong.
void emu_sweep(uint64_t first, uint64_t last, int threads, uint64_t* stats, uint32_t cap, uint32_t* mism, uint32_t* hards,
               uint32_t* wrongs, uint32_t* n_lists) {
    threads = threads < 1 ? 1 : threads;
    std::vector<Tally> ts((size_t)threads);
    std::vector<std::thread> pool;
    const uint64_t per = (last - first + (uint64_t)threads - 1) / (uint64_t)threads;
    for (int i = 0; i < threads; i++) {
        const uint64_t a = std::min(last, first + per * (uint64_t)i), b = std::min(last, a + per);
        pool.emplace_back([a, b, cap, &ts, i] { sweep_range(a, b, cap, ts[(size_t)i]); });
    }
    for (auto& th : pool) th.join();
    Tally all;
    for (const Tally& t : ts) {  // (the threads' ranges ascend: so do the concatenated lists)
        all.mismatches += t.mismatches; all.hard += t.hard; all.audited += t.audited; all.audit_failures += t.audit_failures;
        all.libm_compared += t.libm_compared; all.libm_wrong += t.libm_wrong;
        if (t.libm_max_ulp > all.libm_max_ulp) { all.libm_max_ulp = t.libm_max_ulp; all.libm_max_ulp_arg = t.libm_max_ulp_arg; }
        all.mism.insert(all.mism.end(), t.mism.begin(), t.mism.end());
        all.hards.insert(all.hards.end(), t.hards.begin(), t.hards.end());
        all.wrongs.insert(all.wrongs.end(), t.wrongs.begin(), t.wrongs.end());
    }
    const uint64_t s[8] = {all.mismatches, all.hard, all.audited, all.audit_failures, all.libm_compared, all.libm_wrong,
                           all.libm_max_ulp, all.libm_max_ulp_arg};
    memcpy(stats, s, sizeof s);
    const std::vector<uint32_t>* lists[3] = {&all.mism, &all.hards, &all.wrongs};
    uint32_t* outs[3] = {mism, hards, wrongs};
    for (int k = 0; k < 3; k++) {
        n_lists[k] = (uint32_t)std::min<size_t>(cap, lists[k]->size());
        if (outs[k]) memcpy(outs[k], lists[k]->data(), sizeof(uint32_t) * n_lists[k]);
    }
}
}
