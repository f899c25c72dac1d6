// capi_state.h — what the translation units of the C ABI share (capi.hip, capi_db.hip, capi_psm.hip, capi_host.cpp): the error
// plumbing, the handle structs behind include/sage_hip.h's opaque types, and the few functions that cross files.  Host code only,
// and only those four files include it.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "device_types.h"
namespace sagehip {
int fail(int code, const std::string& msg);  // capi_host.cpp: sets the thread's error string (sage_hip_last_error), returns `code`
}
// a failed HIP call of an entry point (HIP_TRY): the thread's error string is set, the status returned
#define HIP_FAILED(e, what) fail(status_of(e), std::string(what) + ": " + hipGetErrorString(e))
#include "hip_host.h"
#include "host_db.hpp"
#include "localise_math.h"

using namespace sagehip;

// capi_db.hip: the peptide-major fragment list for a batch that takes the stream variant of the preliminary kernels (SageDeviceDb::pm_frag)
int ensure_pm_frag(struct SageDeviceDb* db);

// page-locked host block, grow-only (staging of the streaming pipeline: DMA at full PCIe rate)
struct Pinned {
    unsigned char* p = nullptr;
    size_t cap = 0;
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t reserve(size_t bytes) {
        if (p && bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        const hipError_t e = hipHostMalloc((void**)&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
};

template <class T>
T* carve(unsigned char*& cur, size_t count) {  // next 64-byte aligned array of a staging block
    T* p = (T*)cur;
    cur += ((count * sizeof(T) + 63) / 64) * 64;
    return p;
}

inline uint64_t next_db_serial() {
    static std::atomic<uint64_t> serial{0};
    return ++serial;
}

struct SageHostDb {
    HostDb db;
    // sage_hip_hostdb_isomer_groups: made by the first call (the sizing call), handed out by the ones after it
    mutable std::mutex iso_mu;
    mutable bool iso_made = false;
    mutable std::vector<uint32_t> iso_of, iso_members;
    mutable std::vector<uint64_t> iso_off;
};

struct SageGroupStrings {
    std::vector<std::string> strings;
};

struct SageGroupGraph {
    GroupGraph g;
};

struct SageDeviceDb {
    int device = 0;
    uint64_t serial = next_db_serial();  // never reused: what a batch's stored precursor windows name their index by (WindowKey)
    DevBuf<float> pep_mono;
    DevBuf<uint32_t> pep_lut;  // position table of pep_mono (DevDbView::pep_lut)
    DevBuf<float> ions;
    DevBuf<uint64_t> ion_off;
    DevBuf<uint32_t> pep_info;
    // peptide-major copy: the source of the tile copies while the index is built, afterwards read by the STREAM variant of the
    // preliminary kernels only (windows of a handful of candidates) — released when the build is done (1.16 GB of C3's HBM) and
    // made again, from a tile copy, by the first batch that takes the stream variant (ensure_pm_frag; SAGE_HIP_KEEP_PM_FRAG=1 keeps it)
    DevBuf<SageTheoretical> pm_frag;
    std::mutex pm_mu;
    DevBuf<uint64_t> pm_off;
    std::vector<float> h_pep_mono;    // host copy: window-size estimate at batch upload
    std::vector<uint16_t> h_len;      // host copy of the residue counts: sage_hip_localise_resident's equal-length rule
    DevBuf<SageTheoretical> tm_frag;  // tile-major copy + position table for the large-window kernel
    DevBuf<uint32_t> tm_lut;
    DevBuf<SageTheoretical> tm2_frag; // small-tile copy + table for the narrow kernel's per-peak lookups
    DevBuf<sagecore::LutWord> tm2_l1;  // its position table in succinct form (core.h: LutWord): occupancy + rank per 32 cells ...
    DevBuf<uint32_t> tm2_pos;          // ... and the run starts of the non-empty cells
    uint32_t max_ions = 0;
    uint32_t max_len = 0;   // residues of the longest peptide (> 1023: DevScorer::long_runs)
    uint32_t ion_lo_bits = 0xFFFFFFFFu, ion_hi_bits = 0;  // smallest / largest |ion| of the rescoring table, as f32 bits (scorer_tol_mode)
    DevDbView view{};
    uint64_t bytes = 0;
};

// Device-side working set of ONE scoring pass pair (device_types.h: DevWork).  Kernels of successive batches run in order on
// one compute stream, so a scorer needs a single set whatever the number of batches in flight.
struct WorkSet {
    DevBuf<uint64_t> cand;
    DevBuf<uint32_t> cand_len, totals, status, queue, retry, item_of, ready;
    uint32_t epoch = 0;  // of the last search_kernel launch (DevWork::epoch)
    DevBuf<QueryRec> qrec;
    DevBuf<uint16_t> seeds;
    DevBuf<uint64_t> qres;
    DevBuf<uint32_t> arena;
    // cheap ties (device_types.h: DevWork::cnt_store): the window counts of every narrow single-query spectrum
    DevBuf<uint32_t> cnt_store;
    // the hand-over rows of a narrow first pass (device_types.h: DevWork::hand), one per schedule position
    DevBuf<uint64_t> hand;
    DevBuf<float> winbuf;   // tile_count_wing_kernel's windows (DevWork::winbuf), when a batch needs them
    DevBuf<unsigned char> hugebuf;  // the wide-list kernels' lists in global memory (DevWork::hugebuf), when a configuration needs them
    uint32_t cap_tie = 0;
    uint32_t cap_hand = 0;  // rows `hand` holds
    uint32_t cap_n = 0;     // spectra the narrow-path buffers hold
    uint32_t cap_wide = 0;  // spectra the large-window buffers hold (0 on the second compute lane, always)
};

// What a batch leaves behind: PSM records, counters, timing events.  Double-buffered by the streaming pipeline (batch c + 1 is
// scored while the records of batch c cross PCIe).
struct OutSet {
    DevBuf<SageFeature> features;
    DevBuf<uint32_t> out_count;
    DevBuf<uint32_t> counters;       // [2 * CTR_COUNT]: first pass, exact retry pass
    uint32_t* h_counters = nullptr;  // pinned [2 * CTR_COUNT]
    uint32_t* h_counters_view = nullptr;  // ... as the kernels address it
    bool counters_clean = false;  // the last command on the counters was the epilogue kernel's reset (and the host waited for it)
    Pinned h_out;                    // landing block for the records when the caller's arrays are pageable
    Event ev[5];                     // start, prelim 1, rescore 1, prelim 2, rescore 2
    Event comp_done, down_done;
    bool two_pass = false, with_rescore = false;
    bool wide_launched = true;   // the large-window kernels ran behind it (else: the batch was expected to hold narrow windows only)
    bool timed = true;           // ev[] were recorded for this launch (SageScorer::timing_every)
    bool retry_deferred = false; // two_pass, but the retry pass has not been launched (resident steps: Passes::FirstOnly)
    uint32_t launches[2] = {0, 0};  // what each pass adds to SageTiming::n_launches, counted as it is enqueued (enqueue_first_pass)
    ~OutSet() {
        if (h_counters) (void)hipHostFree(h_counters);
    }
};

struct SageDeviceBatch {
    int device = 0;
    uint32_t n = 0;
    DevBuf<uint64_t> peak_off;
    DevBuf<float> masses, intensities, precursor_mz, iso_lo, iso_hi, tic, rt, ims;
    DevBuf<uint8_t> charge, iso_kind;
    DevBuf<uint32_t> file_id, order, sort_a, sort_b, sort_idx;
    DevBuf<uint8_t> sort_tmp;
    DevBuf<uint4> sched;     // DevBatchView::sched (SAGE_HIP_NO_SCHED=1: not built — the kernels go through `order`)
    WindowKey win_key{};     // resident batches: what the windows in the records' third uint4 were computed from (DevBatchView::sched_key)
    DevBuf<uint8_t> meta;    // streaming pipeline: the per-spectrum arrays in one block, the image of the staging block (one copy)
    uint32_t widest = 0xFFFFFFFFu;  // candidate slots of the batch's widest precursor window (exact_window_check; else unknown)
    bool maybe_wide = true;  // some precursor window may exceed the narrow kernel's LDS counters (estimated at upload; a wrong
                             // "no" is noticed after the step — the queue counter — and the step is repeated with the
                             // large-window kernels)
    Pinned stage;      // host staging of the arrays above (everything but the peaks when those are already page-locked)
    Event up_done;     // uploads of this batch finished (its staging block may be refilled)
    Event sort_done;   // the per-spectrum block is up and the launch schedule sorted (on the scorer's sort stream, beside the peak copies)
    DevBatchView view{};
};

struct SageMzml {
    MzmlRun run;
};

// Scratch of the steps over reported PSMs (capi_psm.hip), grow-only.  The three steps share what they upload alike: one handle
// may annotate, score candidates and localise in any order, each call overwriting what the last one left.
struct PsmScratch {
    DevBuf<SageFeature> feats;  // the features and counts of every step (upload_psms)
    DevBuf<uint32_t> counts;
    // sage_hip_annotate_resident
    DevBuf<uint64_t> an_off;
    DevBuf<uint8_t> an_kinds;
    DevBuf<int32_t> an_charges, an_ord;
    DevBuf<float> an_int, an_calc, an_exp;
    // the candidate lists of sage_hip_score_candidates_resident and sage_hip_localise_resident (upload_candidate_lists)
    DevBuf<uint32_t> cand_list, cand_pep;
    DevBuf<uint64_t> cand_off;
    DevBuf<uint8_t> cand_charge;
    // sage_hip_score_candidates_resident
    DevBuf<SageCandidateScore> cs_out;
    Events<4> cs_ev;  // call begin, kernel begin, kernel end, call end
    float cs_call_ms = 0.f, cs_kernel_ms = 0.f;
    // sage_hip_localise_resident
    DevBuf<SageDepthCounts> lc_counts;
    DevBuf<uint32_t> lc_list2, lc_pair_a, lc_pair_b;
    DevBuf<DevSiteCounts> lc_site;
    Events<6> lc_ev;  // call begin, kernel 1 begin / end, kernel 2 begin / end, call end
    float lc_call_ms = 0.f, lc_kernel_ms = 0.f;
    DepthScores lc_scores;
};

struct SageScorer {
    SageDeviceDb* db = nullptr;
    SageScorerParams params{};
    DevScorer dev{};
    std::mutex mu;                   // entry points taking this handle serialise on it (clone the scorer for concurrency)
    const uint8_t* iso_kind = nullptr;  // the call in progress (under `mu`): SAGE_TOL_* of each spectrum's isolation window, null = Da
    hipStream_t stream = nullptr;    // compute (and, for resident batches, the result download)
    hipStream_t up_stream = nullptr, down_stream = nullptr;  // streaming pipeline: H2D of batch c + 1, D2H of batch c - 1
    hipStream_t side_stream = nullptr;  // kernels of one batch that may run next to each other (the two heap-replay kernels); also the
                                        // per-spectrum block + launch-schedule sort of an UPLOADING batch, beside its peak copies
                                        // (stage_and_upload).  Not a stream of its own for that: one more stream per scorer changed
                                        // how HIP maps streams to hardware queues and the two parts of a small resident step
                                        // (way streams) stopped overlapping — 62 500 C3 spectra: 0.79 -> 0.98 ms.
    Event side_fork, side_join;
    // a resident narrow-search step in `ways` parts, each with its own stream (part 0: `stream`): the parts' kernels overlap each
    // other's cold starts, tails and retry chains (what two scorer handles on two host threads get, inside one call)
    uint32_t ways = 0;               // SAGE_HIP_WAYS=1..4; 0: by batch size (resident_attempt).  Measured on C3: two parts
                                     // -1 % wall at 500 000 spectra, -6 % at 62 500, nothing more with three or four
    hipStream_t way_stream[3] = {nullptr, nullptr, nullptr};
    Event way_begin, way_end[4];  // (way_end[p]: behind the last command of part p)
    DevBuf<uint32_t> win_max;   // exact_window_check's result word
    bool retry_likely = true;   // the last resident step had spectra to retry (or there was none yet): the next one launches its
                                // retry pass unconditionally
    // per-kernel HIP events of a step (SageTiming::prelim_ms / rescore_ms / retry_ms): on every `timing_every`-th scoring call
    // (sage_hip_scorer_set_timing_interval; 1: every call, 0: never).  Eight event records and six elapsed-time queries cost a
    // 0.65 ms step ~15 us; a step without them reports the last timed step's kernel times.
    uint32_t timing_every = 1;
    uint64_t timing_calls = 0;
    bool timed = true;          // this call records events
    float kept_prelim_ms = 0.f, kept_rescore_ms = 0.f, kept_retry_ms = 0.f;
    DevBuf<double> lnfact;
    DevBuf<unsigned long long> dbg;  // SAGE_HIP_PHASE_CLOCKS=1: per-phase cycle accumulators
    uint32_t tile_blocks = 0;        // persistent workgroups of the large-window kernel (u16 counters)
    uint32_t tile_blocks8 = 0;       // ... of its u8 instance (smaller LDS footprint: more of them per CU)
    bool cnt8 = true;                // first pass of a search counts in u8 (SAGE_HIP_NO_U8=1 turns it off)
    bool reuse_counts = true;        // the retry pass reuses the first pass's large-window counts (SAGE_HIP_NO_REUSE=1 turns it off)
    SageTiming timing{};
    bool exact_always = false;  // SAGE_HIP_EXACT=1: never use the order-free trims
    bool one_launch = false;    // SAGE_HIP_ONE_LAUNCH=1: the first pass of narrow windows as one launch of two kinds of workgroups
                                // (kernels.hip: search_kernel) instead of prelim_kernel, then rescore_kernel — measured slower, like
                                // the fused kernel: the larger kernel body costs scalar-register spills
    uint32_t kstride = 64;           // entries per query of the large-window pipeline's seed / heap arrays (DevWork::kstride)
    bool two_lanes = true;           // streaming pipeline: two chunks of a narrow batch side by side (SAGE_HIP_ONE_LANE=1: one at a time)
    uint32_t search_lag = 0;         // SAGE_HIP_SEARCH_LAG (DevWork::search_lag)
    bool sched_desc_forced = false;  // SAGE_HIP_SCHED_DESC was given (else: heaviest precursors first for narrow batches only)
    uint64_t replay_split = 0xFFFFFFFFull;  // SAGE_HIP_REPLAY_WAVE_MAX | SAGE_HIP_REPLAY_LANE_MAX << 32 (DevWork::replay_split); default: every query by wavefront
    bool fused = false;         // SAGE_HIP_FUSED=1: the first pass of narrow windows through the fused kernel as well (measured slower
                                // than the two kernels on MI355X — register pressure, DESIGN.md 4.7 — kept for that comparison)
    bool zero_copy = true;      // records go straight to page-locked result arrays (SAGE_HIP_NO_ZEROCOPY=1: device buffer + copy)
    bool fast_ties = true;      // one reported PSM, no chimera: ties at the top settled by rescore_kernel from stored window counts
                                // (SAGE_HIP_NO_FAST_TIES=1: every tie through the exact retry pass, as in round 3)
    uint32_t cnt_stride = 0;    // words per spectrum of WorkSet::cnt_store
    bool hand_rows = true;      // the narrow first pass hands its lists over in schedule order (DevWork::hand) where plan_step
                                // allows it (SAGE_HIP_DEBUG_FLAGS=131072, read at scorer creation: always by spectrum)
    bool last_hand = false;     // ... and the last first pass enqueued did (sage_hip_debug_handover_route)
    uint32_t last_rescore = RESCORE_INST_NONE;  // the rescoring instance the last first pass (or quick_score) launched (sage_hip_debug_rescore_instance)
    uint32_t qmax = 1;
    WorkSet ws;                 // the working set (lane 0)
    WorkSet ws2;                // a second one: the streaming pipeline scores two chunks of a narrow batch side by side (lane 1)
    OutSet outs[4];             // [k % 4]: the slots of the streaming pipeline; [0..ways): the concurrent parts of a resident step
    SageDeviceBatch slots[4];   // input buffers of the streaming pipeline (chunk k in slot k % 4: uploads run ahead of the kernels)
    uint32_t chunk = 131072;    // spectra per pipeline stage (SAGE_HIP_CHUNK): 39.9 M spectra/s host to host on C3 against 38.2 M at 65 536 and 37.3 M at 262 144
    DevBuf<uint8_t> keep;       // scratch of sage_hip_quick_score_resident, grow-only
    PsmScratch psm;
};
