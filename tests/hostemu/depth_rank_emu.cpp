// Host build of the depth ranks and the min-rank of a tolerance window (sage_amd/csrc/core.h: depth_rank_of,
// min_rank_in_window_lockstep) — what depth_counts_kernel and site_counts_kernel of kernels.hip count with —
// behind a tiny C ABI for tests/test_depth_rank_emulation.py, which holds them to the plain restatement of
// tests/localise_reference.py.  TEST INFRASTRUCTURE.
#include <cstdint>

#include "../../sage_amd/csrc/core.h"

using namespace sagecore;

extern "C" {

// ranks[p] of every peak, one call of depth_rank_of per peak as the kernels make it per lane
void emu_depth_ranks(const float* masses, const float* intensities, uint32_t n, uint8_t* ranks) {
    for (uint32_t p = 0; p < n; p++) ranks[p] = depth_rank_of(masses, intensities, n, p);
}

uint32_t emu_min_rank(const float* masses, const uint8_t* ranks, uint32_t n, float center, int tol_kind, float tol_lo, float tol_hi) {
    const Tol tol{tol_kind, tol_lo, tol_hi};
    return min_rank_in_window_lockstep(masses, ranks, n, pow2_floor(n), center, tol);
}

// the peak select_most_intense_peak_lockstep picks for the same window (-1: none): the two searches look at the same peaks
int emu_most_intense(const float* masses, const float* intensities, uint32_t n, float center, int tol_kind, float tol_lo, float tol_hi) {
    const Tol tol{tol_kind, tol_lo, tol_hi};
    return select_most_intense_peak_lockstep(masses, intensities, n, pow2_floor(n), center, tol);
}

uint32_t emu_depth_constants(uint32_t which) { return which == 0 ? DEPTH_RANK_CAP : which == 1 ? DEPTH_NO_PEAK : DEPTHS; }

}  // extern "C"
