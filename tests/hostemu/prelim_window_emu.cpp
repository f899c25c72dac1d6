// Host build of the one-thread precursor-window search whose result a resident batch keeps in its schedule records
// (sage_amd/csrc/core.h: scalar_query_window) — behind a tiny C ABI for tests/test_prelim_window_emulation.py.  TEST INFRASTRUCTURE.
#include <cstdint>

#include "../../sage_amd/csrc/core.h"

using namespace sagecore;

extern "C" {

// out[4] = {left, right, first, end}
void emu_scalar_query_window(const float* pep_mono, uint32_t np, float plo, float phi, uint32_t* out) {
    const Window q = scalar_query_window(pep_mono, np, plo, phi);
    out[0] = q.left;
    out[1] = q.right;
    out[2] = q.first;
    out[3] = q.end;
}

int32_t emu_order_key(float f) { return order_key(f); }

}  // extern "C"
