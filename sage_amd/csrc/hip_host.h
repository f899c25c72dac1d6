// Host-side owners of HIP resources and the error plumbing the .hip files share.  Host code only: kernels.hip does not include it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sage_hip.h"
#include "core.h"

namespace sagehip {

inline int status_of(hipError_t e) { return e == hipErrorOutOfMemory ? SAGE_HIP_ERR_OOM : SAGE_HIP_ERR_HIP; }

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        release();
        n = count;
        return hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
    }
    hipError_t upload(const T* src, size_t count) {
        hipError_t e = alloc(count);
        if (e != hipSuccess) return e;
        return count ? hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    }
    // grow-only: keep the allocation when it is large enough (no driver call on the steady-state path)
    hipError_t reserve(size_t count) {
        if (p && count <= n) return hipSuccess;
        return alloc(std::max(count, n + n / 2));
    }
    size_t bytes() const { return n * sizeof(T); }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t create(bool timing) { return e ? hipSuccess : hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming); }
};

template <int N>
struct Events {  // the timing events of one call, created in index order
    Event at[N];
    hipError_t create() {
        hipError_t e = hipSuccess;
        for (int i = 0; i < N && e == hipSuccess; ++i) e = at[i].create(true);
        return e;
    }
    hipEvent_t operator[](int i) const { return at[i].e; }
};

struct Stream {  // a non-blocking stream created for one call
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

// What a call on the device carries through its helpers: its stream, and the status and message of its first failure.
struct Ctx {
    hipStream_t stream = nullptr;
    std::string err;
    int code = SAGE_HIP_OK;
    const char* prefix = "";  // of the message of a failed HIP call ("sage_hip_lfq: ")
    bool fail(int c, std::string msg) {
        code = c;
        err = std::move(msg);
        return false;
    }
    bool check(hipError_t e, const char* what) { return e == hipSuccess || fail(status_of(e), std::string(prefix) + what + ": " + hipGetErrorString(e)); }
};

// HIP_TRY(expr): when the HIP call fails, return HIP_FAILED(error, "expr") from the enclosing function.  By default that notes the
// failure in the Ctx named cx and returns false.  A file whose functions return something else defines HIP_FAILED before it
// includes this header: capi_state.h (the status, with the thread's error string set), index_build.hip (the hipError_t itself).
#ifndef HIP_FAILED
#define HIP_FAILED(e, what) cx.check((e), (what))
#endif
#define HIP_TRY(expr)                                             \
    do {                                                          \
        const hipError_t _e = (expr);                             \
        if (_e != hipSuccess) return HIP_FAILED(_e, #expr);       \
    } while (0)

// The entry of a whole-call product (sage_hip_rescore, _predict_rt, _protein_groups, _lfq): choose the device, create the call's
// stream, run body(cx) on it, wait for the stream, and turn a failure into the status and `err`.  `name` heads the message of a
// failed hipSetDevice, `prefix` is Ctx::prefix.  A Scope is constructed from (device, stream) before the body and destroyed when
// the call returns: post_search.h's ScratchScope for the calls that allocate from the pool.
struct NoScope {
    NoScope(int, hipStream_t) {}
};
template <class Scope = NoScope, class Body>
int run_on_device(int device, const char* name, const char* prefix, std::string& err, Body&& body) {
    Ctx cx;
    cx.prefix = prefix;
    if (hipSetDevice(device) != hipSuccess) {
        err = std::string(name) + ": hipSetDevice failed";
        return SAGE_HIP_ERR_NO_DEVICE;
    }
    Stream stream;
    if (!cx.check(stream.create(), "hipStreamCreate")) {
        err = cx.err;
        return cx.code;
    }
    cx.stream = stream.s;
    Scope scope(device, cx.stream);
    const bool ok = body(cx);
    (void)hipStreamSynchronize(cx.stream);
    if (!ok) {
        err = cx.err;
        return cx.code ? cx.code : SAGE_HIP_ERR_HIP;
    }
    return SAGE_HIP_OK;
}

// rocPRIM's two-call protocol: call(nullptr, bytes) asks for the size of the scratch, call(scratch, bytes) runs in it.  `tmp` (a
// DevBuf, or post_search.h's pooled Buf) has to outlive the work, so it is the caller's — or, in the second form, freed on return.
template <class Scratch, class Call>
hipError_t with_scratch(Scratch& tmp, Call&& call) {
    size_t bytes = 0;
    hipError_t e = call((void*)nullptr, bytes);
    if (e == hipSuccess) e = tmp.alloc(bytes);
    if (e == hipSuccess) e = call((void*)tmp.p, bytes);
    return e;
}
template <class Scratch, class Call>
hipError_t with_scratch(Call&& call) {
    Scratch tmp;
    return with_scratch(tmp, call);
}

// index_build.hip (each returns a hipError_t); the outputs are allocated there, their `n` is the table's length
// A tile-major copy of the peptide-major list for tiles of 2^tile_shift peptides + its position table (lut_stride cells per tile)
int build_tile_copy_on_device(const SageTheoretical* d_pm_frag, uint64_t nf, uint32_t tile_shift, uint32_t n_tiles,
                              const uint64_t* d_tile_off, float lut_scale, SageTheoretical* d_tm_frag, DevBuf<uint32_t>& lut,
                              uint32_t* lut_stride_out, void* stream);
// lut[n_tiles][lut_stride] (row-major, as build_tile_copy_on_device makes it) -> its succinct form
int build_succinct_lut_on_device(const uint32_t* d_lut, uint32_t n_tiles, uint32_t lut_stride, DevBuf<sagecore::LutWord>& l1,
                                 DevBuf<uint32_t>& pos, uint32_t* words_out, void* stream);
int build_peptide_mass_lut(const float* d_pep_mono, uint32_t np, float top_mass, DevBuf<uint32_t>& lut, uint32_t* bins_out, float* inv_w_out,
                           void* stream);

// process.hip: SpectrumProcessor::process of every spectrum of `raw`, enqueued on cx.stream (sage_hip_batch_process_upload and the
// MS2 path of sage_hip_tmt).  `w` holds the inputs and intermediates until the caller's stream is done with them.
struct ProcessScratch {
    DevBuf<uint64_t> raw_off;
    DevBuf<float> raw_mz, raw_int, sm, si;
    DevBuf<uint8_t> zbuf;
    DevBuf<uint32_t> cnt, big_list;
    DevBuf<unsigned char> big_ws;
};
bool process_raw_on_device(Ctx& cx, const SageRawBatch* raw, uint64_t take_top_n, int deisotope, float min_deisotope_mz, uint32_t min_peaks,
                           ProcessScratch& w, DevBuf<uint64_t>& peak_off, DevBuf<float>& masses, DevBuf<float>& intensities,
                           DevBuf<float>& tic, std::vector<uint32_t>& counts, std::vector<uint64_t>& off);

}  // namespace sagehip
