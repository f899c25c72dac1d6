// purity.h — the definition of the precursor purity of a reported PSM, shared by the device (purity.hip) and the
// host (tests/hostemu/purity_emu.cpp compiles it by itself).  How much of the ion beam that the instrument isolated for an MS2
// scan was the identified precursor, read off one MS1 spectrum: the intensity inside the isolation window that lies on the
// precursor's isotope envelope, over all the intensity inside the window.  An addition over the reference.
//
// A query is a precursor m/z `mz`, a charge `z` (0: unknown), isolation offsets (lo, hi) in Da (either NaN: the settings' default
// pair) and one MS1 spectrum, whose peaks are raw m/z, read in the order given:
//   window    wlo = mz + lo, whi = mz + hi; a peak is IN THE WINDOW iff wlo <= p.mz && p.mz <= whi (a NaN m/z never is)
//   envelope  c_k = mz + (k * NEUTRON) / z for k = 0 .. max_isotope (z == 0: only c_0 = mz); (elo_k, ehi_k) = the ppm bounds of c_k
//             (tol_bounds); a peak in the window is MATCHED iff it lies inside the bounds of at least one k (counted once)
//   below     c_below = mz - NEUTRON / z with its ppm bounds; EVERY peak of the spectrum inside them counts, in the window or not
//             (z == 0: none).  A large `below` says the instrument picked an isotope peak, not the monoisotopic one.
//   sums      total (in the window), matched (in the window and matched), below: f64, each from +0.0, each adding
//             (double)p.intensity over its peaks ONE AFTER ANOTHER IN ASCENDING POSITION.  The order is part of the contract;
//             NaN, +-inf, negative and -0.0 intensities pass through as written.
//   purity    (float)(matched / total), the division in f64, stored as computed (0 / 0 included); -1.0f when no peak is in the
//             window or the query has no MS1 spectrum, with all sums (`below` too) +0.0 and all counts 0.
// All m/z arithmetic is f32, one rounding per operation (-ffp-contract=off on every translation unit that includes this file).
#pragma once
#include <stdint.h>

#include "core.h"

namespace purity {

constexpr uint32_t MAX_ISOTOPE = 16;            // the largest max_isotope a call accepts
constexpr uint64_t NO_MS1 = ~(uint64_t)0;       // ms1_index of a query without an MS1 spectrum

struct Settings {
    float ppm_tolerance, default_lo, default_hi;
    uint32_t max_isotope;
};

struct Result {
    uint32_t n_window, n_matched;
    double total, matched, below;
    float purity;
};

SAGE_HD sagecore::Tol ppm_tol(float t) { return sagecore::Tol{0, -t, t}; }

// the isolation window of a query
SAGE_HD void window_bounds(float mz, float lo, float hi, const Settings& st, float& wlo, float& whi) {
    if (lo != lo || hi != hi) {
        lo = st.default_lo;
        hi = st.default_hi;
    }
    wlo = mz + lo;
    whi = mz + hi;
}
SAGE_HD bool inside(float lo, float hi, float p) { return lo <= p && p <= hi; }

// the ppm bounds of the k-th centre of the envelope; (NaN, NaN) — no peak is inside — where the centre does not exist
SAGE_HD void envelope_bounds(float mz, uint32_t z, uint32_t k, const Settings& st, float& lo, float& hi) {
    lo = hi = __builtin_nanf("");
    if (k > st.max_isotope || (z == 0 && k > 0)) return;
    float c = mz;
    if (z != 0) {
        const float d = ((float)k * sagecore::NEUTRON) / (float)z;
        c = mz + d;
    }
    sagecore::tol_bounds(ppm_tol(st.ppm_tolerance), c, lo, hi);
}
// the ppm bounds of the position one neutron below the precursor; (NaN, NaN) for an unknown charge
SAGE_HD void below_bounds(float mz, uint32_t z, const Settings& st, float& lo, float& hi) {
    lo = hi = __builtin_nanf("");
    if (z == 0) return;
    const float d = sagecore::NEUTRON / (float)z;
    const float c = mz - d;
    sagecore::tol_bounds(ppm_tol(st.ppm_tolerance), c, lo, hi);
}

SAGE_HD Result no_result() { return Result{0u, 0u, 0.0, 0.0, 0.0, -1.0f}; }
// the last step of a query: purity from the sums, or the result of a query without a peak in its window
SAGE_HD Result finish(uint32_t n_window, uint32_t n_matched, double total, double matched, double below) {
    if (!n_window) return no_result();
    return Result{n_window, n_matched, total, matched, below, (float)(matched / total)};
}

// One query over one spectrum, peak after peak: the definition as one caller runs it.
SAGE_HD Result evaluate(const float* mz_of, const float* intensity_of, uint64_t n, float mz, uint32_t z, float lo, float hi,
                        const Settings& st) {
    Result r = no_result();  // (the sums and counts start from its zeros)
    float wlo, whi, blo, bhi;
    window_bounds(mz, lo, hi, st, wlo, whi);
    below_bounds(mz, z, st, blo, bhi);
    for (uint64_t i = 0; i < n; ++i) {
        const float p = mz_of[i];
        const double v = (double)intensity_of[i];
        if (inside(blo, bhi, p)) r.below += v;
        if (!inside(wlo, whi, p)) continue;
        ++r.n_window;
        r.total += v;
        bool hit = false;
        for (uint32_t k = 0; k <= st.max_isotope && !hit; ++k) {
            float elo, ehi;
            envelope_bounds(mz, z, k, st, elo, ehi);
            hit = inside(elo, ehi, p);
        }
        if (hit) {
            ++r.n_matched;
            r.matched += v;
        }
    }
    return finish(r.n_window, r.n_matched, r.total, r.matched, r.below);
}

}  // namespace purity
