// Plain-data views passed by value to the HIP kernels (kernels.hip) by the C-ABI layer (capi.hip).
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/sage_hip.h"
#include "core.h"

namespace sagehip {

// Device-resident database.
struct DevDbView {
    const float* pep_mono;        // [np]   peptide masses, ascending — the precursor-window search key
    uint32_t np;
    // ... and its position table (index_build.hip: build_peptide_mass_lut): pep_lut[b] = first peptide with mass >= b / pep_lut_inv_w
    // in the total order, b = 0..pep_lut_bins (pep_lut[pep_lut_bins] == np); pep_lut_bins == 0: none
    const uint32_t* pep_lut;
    uint32_t pep_lut_bins;
    float pep_lut_inv_w;
    // peptide-major copy of IndexedDatabase.fragments: the same (peptide_index, fragment_mz) entries grouped by
    // peptide, so that a precursor window is ONE contiguous, coalesced range (narrow kernel, small windows)
    const SageTheoretical* pm_frag;  // [nf]
    const uint64_t* pm_off;          // [np + 1]
    // complete ion table for rescoring: ions[ion_off[p] + k*(L-1) + idx] = IonSeries(p, kinds[k])[idx]
    const float* ions;
    const uint64_t* ion_off;         // [np + 1]
    const uint32_t* pep_info;        // [np] len | decoy<<16 | missed_cleavages<<24
    // tile-major copy of the fragments for large precursor windows: tile = peptide_index >> tile_shift,
    // ascending m/z inside a tile, plus a per-tile position table:
    //   tm_lut[tm_lut_index(t, c)] = position in tm_frag of tile t's first fragment with m/z >= c / lut_scale
    // (the last cell of a tile is its end position), row-major: lut[t][c].  (Round 4 measured the transposed layout, lut[c][t] —
    // the words one fragment-tolerance window needs from the ~100 consecutive tiles of a precursor window share cache lines:
    // same kernel time, 16 % MORE HBM traffic on C4 (2.48 against 2.13 MB per spectrum: a tile's windows no longer share the
    // tile's row).)  A (peak window, tile) lookup is two table reads and a
    // short contiguous run of entries; the tile's candidate counters fit in LDS.
    const SageTheoretical* tm_frag;  // [nf + 2]
    const uint32_t* tm_lut;          // [n_tiles * lut_stride]
    uint32_t tile_shift;
    uint32_t n_tiles;
    uint32_t lut_stride;
    float lut_scale;
    // a second tile-major copy with SMALL tiles (2^tile2_shift peptides, coarser cells) for the narrow kernel's per-peak
    // lookups: a +-10 ppm window holds a few hundred candidates, and a run of a small tile is ~3 entries instead of ~30
    const SageTheoretical* tm2_frag;  // [nf + 2]
    // its position table in succinct form (core.h: LutWord / lut_rank): lut2_words words per tile, each {occupancy bits of 32 cells,
    // rank = index into tm2_pos of the first non-empty cell at or after the word's first cell}; tm2_pos: the run starts of a tile's
    // non-empty cells in cell order, then the tile's end
    const sagecore::LutWord* tm2_l1;  // [n_tiles2 * lut2_words]
    const uint32_t* tm2_pos;          // [non-empty cells of all tiles + n_tiles2]
    uint32_t lut2_words;              // ceil(lut2_stride / 32)
    uint32_t tile2_shift;
    uint32_t n_tiles2;
    uint32_t lut2_stride;
    float lut2_scale;
    uint64_t nf;
    uint8_t ion_kinds[8];
    uint32_t n_kinds;
};

// Layout of the large tiles' position table (tm_lut): row-major, lut[t][c], n_tiles rows.  (The transposed layout, lut[c][t], of
// round 4 and the quads of tiles, lut[t / 4][c][t % 4], of round 5 measured no better: DESIGN.md 4.2.)
constexpr uint32_t TILE_SHIFT_MAX = 15;  // the large tiles hold at most 2^15 peptides (the count kernel's scan: 64 slots per thread)
__host__ __device__ inline size_t tm_lut_index(uint32_t t, uint32_t c, uint32_t lut_stride) { return (size_t)t * lut_stride + c; }

// SAGE_HIP_PHASE_CLOCKS=1: DevWork::dbg holds DBG_BLOCKS rows of 32 words (phase cycles and byte counts, kernels.hip: PhaseClock)
// and behind them DBG_BLOCKS rows of DBG_PRUNE_WORDS words: what the rescoring prune dropped (words 0..3, sage_hip_debug_prune_counters)
// the trips of the bitmap filter's two routes (words 4..7, sage_hip_debug_filter_counters) and what the cooperative path of the heavy
// candidates took (words 8..9, sage_hip_debug_heavy_counters) and by which route (words 10..11, sage_hip_debug_heavy_routes)
constexpr uint32_t DBG_BLOCKS = 4096, DBG_PRUNE_WORDS = 12;
constexpr size_t DBG_TOTAL_WORDS = (size_t)DBG_BLOCKS * (32 + DBG_PRUNE_WORDS);

struct DevScorer {
    sagecore::Tol precursor_tol, fragment_tol;
    sagecore::PbmReach pbm_reach;  // pbm_reach_of(fragment_tol): the peak-presence bitmap's reach coefficients (core.h)
    uint32_t min_matched_peaks;
    int min_isotope_err, max_isotope_err;
    uint32_t min_precursor_charge, max_precursor_charge;
    uint32_t override_precursor_charge;
    int max_fragment_charge;  // -1 == None
    uint32_t chimera;
    uint32_t report_psms;
    uint32_t wide_window;
    int score_type;
    uint32_t kmax;       // max(50, 2*report_psms): upper bound of every trim_k()
    uint32_t big_path;   // 1: the instances for lists wider than a wavefront (report_psms > 32: heaps in LDS, every trim exact,
                         //    rescore_big_kernel) — also taken by a database with peptides of more than 1023 residues, whose
                         //    Run states need the two-register form (long_runs; core.h: run_matched_packed)
    uint32_t long_runs;  // 1: ion indices beyond 1023 occur
    uint32_t tol_mode;   // core.h: TolMode bits — how the rescoring kernels may evaluate Tolerance::bounds of a fragment and the m/z of
                         //    a charge-3 fragment (capi.hip: scorer_tol_mode)
    uint32_t list_cap;   // capacity (entries) of each of the two CLists
    uint32_t wcap;       // candidate-slot capacity of the LDS counter array of the narrow kernel: spectra with a
                         // larger precursor window go to the tiled large-window kernel
    uint32_t dbg_flags;  // timing experiments only (SAGE_HIP_DEBUG_FLAGS)
    uint32_t prune_min;  // min_matched_peaks for the rescoring kernels' prune (kernels.hip: score_candidates drops a candidate that cannot
                         //    reach it any more, rescore_spectrum leaves when no candidate reached it); 0: both off (SAGE_HIP_DEBUG_FLAGS=4096)
    uint32_t rescore_general;  // host only, decided at scorer creation; bits (RESCORE_GENERAL_*):
                               //    1: launch_rescore takes the general instance of rescore_kernel (CHIMERA == true) for every search
                               //       (SAGE_HIP_RESCORE_GENERAL=1: tests and A/B runs of the two routes)
                               //    2: ... and never the instance compiled for two ion kinds (KINDS2): the database's kinds are not
                               //       {n-terminal, other}, or SAGE_HIP_RESCORE_KINDS_GENERAL=1
    uint32_t xcd_chunk;  // consecutive schedule positions one XCD takes at a time (kernels.hip: xcd_position); 0: round-robin
    uint32_t fast_log;   // 1: this pass is followed by the exact retry pass, so its rescoring kernel may carry the fast phase of the
                         //    correctly rounded logarithm only and queue the (rare) spectrum it cannot round for (crlog.h)
    uint32_t exact;      // 1: every trim_hits replays bounded_min_heapify, so the preliminary list has the reference's heap
                         //    layout.  0: each trim keeps the same SET of candidates (the k largest) without replaying the
                         //    heap; the layout is only observable through equal hyperscores at a reported rank, which the
                         //    rescoring kernel detects and sends back through the exact path
};

struct DevBatchView {
    uint32_t n;                 // spectra of this batch == upper bound of the launch grids
    const uint32_t* n_dev;      // when not null: the number of entries of `order` to score lives on the device (the exact
                                //     retry pass is launched without a host round trip: its count is a counter of pass 1)
    uint32_t spec_base;         // added to Feature.spec_index: position of this batch's first spectrum in the caller's batch
    const uint64_t* peak_off;
    const float* masses;
    const float* intensities;
    const float* precursor_mz;
    const uint8_t* precursor_charge;
    const float* isolation_lo;  // may be null
    const float* isolation_hi;
    const float* tic;
    const float* rt;            // may be null
    const float* ims;           // may be null
    const uint32_t* file_id;    // may be null
    const uint32_t* order;      // [n] block b scores spectrum order[b]: ascending precursor mass => neighbouring
                                //     wavefronts stream overlapping index ranges (L2 reuse); results stay in input order
    uint32_t probe;             // narrow kernel variant: 1 = per-peak table lookups (large windows), 0 = peptide-major stream
    uint32_t pcap;              // max peaks per spectrum in this batch
    uint32_t fzcap;             // max (max_fragment_charge - 1) over the charges this batch can use
    const uint4* sched;         // may be null.  [sched_stride n] what a block needs of the spectrum it scores, IN SCHEDULE ORDER: record b =
                                //     {order[b], peaks, peak_off lo, hi}, {charge, precursor m/z, isolation lo, hi (NaN: none)} — one
                                //     trip to a line its neighbours share instead of order[b] and then five random reads.  The
                                //     charge word carries (SAGE_TOL_* of the isolation window) ^ SAGE_TOL_DA in bits 8-15: 0 for Da
    const uint8_t* iso_kind;    // may be null (every window Da): SAGE_TOL_* of isolation_lo / hi (MGF `TOLU=ppm`)
    uint32_t sched_stride;      // uint4 per record of `sched`: SCHED_RECORD, or SCHED_RECORD_WINDOW for a resident batch, whose upload leaves {left, right, first,
                                //     end} of the spectrum's FIRST precursor-window query (kernels.hip: window_max_kernel) in the third
    uint32_t sched_win;         // 1: the third uint4 is there AND belongs to the scorer of this launch (capi.hip: WindowKey): the
                                //     preliminary kernel takes the window from it instead of searching
    const struct WindowKey* sched_key;  // host only: what the records' windows were computed from (null: no windows)
};
// uint4 per schedule record (DevBatchView::sched_stride): the two every record has, and those of a resident batch, whose third
// holds the window of the spectrum's first precursor-window query
constexpr uint32_t SCHED_RECORD = 2, SCHED_RECORD_WINDOW = 3;
// What a precursor window depends on besides the spectrum: a batch's stored windows hold for a scorer with the same key only
// (a device batch may be scored by any handle).
struct WindowKey {
    uint64_t db_serial;  // SageDeviceDb::serial
    sagecore::Tol precursor_tol;
    uint32_t wide_window, min_precursor_charge, max_precursor_charge, override_precursor_charge;
    int min_isotope_err, max_isotope_err;
};

struct DevWork {  // per-spectrum outputs of the preliminary pass
    uint64_t* cand;        // [n * kmax] packed PreScore in the reference's heap-layout order
    uint32_t* cand_len;    // [n]
    uint32_t* totals;      // [n * 2] InitialHits.matched_peaks, .scored_candidates
    uint32_t* status;      // [n] 0 ok, 1 deferred to the large-window kernel, 2 list overflow
    uint32_t* n_deferred;  // [8]: [0] spectra queued for the large-window kernels, [1] list overflows,
                           //      [2] queue head (next entry a large-window workgroup takes),
                           //      [3] candidate-arena bump pointer, [4] candidate-arena overflows
    uint32_t* queue;       // [n] spectra queued for the large-window kernels
    uint32_t* retry;       // [n] spectra whose reported ranks tie in hyperscore: re-run with exact heap layouts
    uint32_t tile_blocks;  // persistent workgroups of the large-window counting kernel
    uint32_t cnt8;         // count in u8 (first pass of a two-pass search only: overflowing spectra go to the u16 retry pass)
    uint32_t reuse;        // retry pass: the large-window counts of the first pass are reused through item_of (kernels.hip: query_slot)
    uint32_t queue_later;  // prelim_kernel only marks a spectrum it hands to the large-window kernels (status); queue_kernel appends the
                           //     marked ones to `queue` behind it, a wavefront's worth per atomic (kernels.hip: queue_kernel)
    uint32_t* item_of;     // [n] spectrum -> its item in the first pass's queue; bit 31: count again (a u8 counter may have wrapped)
    uint32_t* ready;       // [n] search_kernel: == epoch once the spectrum's preliminary list is in HBM (written with agent-scope release)
    uint32_t epoch;        //     of this launch (never 0; the array is zeroed when it is allocated)
    uint64_t replay_split; // which heap-replay kernel takes a query: low 32 bits = queries up to which every query gets a wavefront
                           //     (SAGE_HIP_REPLAY_WAVE_MAX; default 0xFFFFFFFF: every query, the lane-per-query kernel is not launched), high 32 bits = stream words above which a query does
                           //     anyway (SAGE_HIP_REPLAY_LANE_MAX, 0: the default of kernels.hip)
    uint32_t kstride;      // entries per query of `seeds` / `qres`: kmax rounded up to a multiple of 64 (64 unless report_psms > 32)
    uint32_t search_lag;   //     workgroup ids by which a spectrum's rescoring trails its preliminary workgroup (0: the default)
    // Cheap ties (kernels.hip: rescore_spectrum).  The preliminary kernel leaves the window counts of every narrow single-query
    // spectrum in HBM; where the hyperscores of a spectrum's best candidates tie (and report_psms == 1, no chimera), the rescoring
    // wavefront replays bounded_min_heapify from them on the spot, finds which of the tied candidates comes first in the
    // reference's preliminary list and reports it — instead of queueing the spectrum for the exact retry pass.
    uint32_t* cnt_store;   // [n * cnt_stride] one row per SCHEDULE POSITION of the launch (null: off): {left, potential, -, -} of the
                           //     spectrum's query — potential == 0: nothing kept (several queries, large window) — then its u16
                           //     counts in slot order, two per word
    uint32_t cnt_stride;   //     words per row (4 + wcap / 2, a multiple of 4)
    uint32_t* arena_ptr;   // the arena's bump pointer (the first pass's counter in both passes when the retry pass reuses its candidates)
    // large-window pipeline (count -> replay -> assemble); query id = queue position * qmax + (z - z0) * n_iso + iso index
    struct QueryRec* qrec; // [n * qmax]
    uint16_t* seeds;       // [n * qmax * kstride] matched counts of the first min(k, potential) candidate slots
    uint64_t* qres;        // [n * qmax * kstride] heap of each k-selected query, in the reference's layout order
    unsigned char* hugebuf;  // non-null: the lists / heaps / per-candidate arrays of the wide-list kernels (report_psms > 32) in global
    uint32_t huge_stride;    //     memory, [huge_grid()] slices of huge_stride bytes, one per workgroup (they no longer fit a CU's LDS)
    float* winbuf;         // non-null: tile_count_wing_kernel — [tile_blocks][2][fzcap * pcap] the spectrum's windows in global memory
    uint32_t* arena;       // candidate segments: {next, n, tile_base, 0} then n entries `count << 16 | slot in tile`
    uint32_t arena_cap;    // entries
    uint32_t qmax;
    uint32_t tile_shift;   // log2 of the peptides per tile (the readers of the candidate directories need it)
    unsigned long long* dbg;  // optional [2][8] per-phase cycle accumulators (null in production)
    // The hand-over of a narrow first pass in SCHEDULE order (null: off — cand / cand_len / totals / status by spectrum, as every other
    // route).  [n * HAND_ROW_WORDS] one 512-byte row per schedule position of the launch: prelim_kernel writes the row of every
    // position, rescore_kernel reads it beside the schedule record instead of behind it.
    uint64_t* hand;
};
// A row of DevWork::hand: the packed PreScore list in words 0 .. kmax - 1 (what goes to `cand` on the other routes), then
// {status, stored} and {matched_peaks, scored_candidates} — low word first — in the last two words.  One word per lane.
constexpr uint32_t HAND_ROW_WORDS = 64, HAND_HEAD_WORD = 62, HAND_TOTALS_WORD = 63, HAND_LIST_MAX = HAND_HEAD_WORD;
static_assert(HAND_LIST_MAX <= HAND_HEAD_WORD && HAND_HEAD_WORD < HAND_TOTALS_WORD && HAND_TOTALS_WORD < HAND_ROW_WORDS && HAND_ROW_WORDS == 64,
              "the list and the two header words fit a row of one word per lane");
static_assert(HAND_ROW_WORDS * sizeof(uint64_t) % 128 == 0, "rows keep the array's 128-byte alignment");

enum { ST_OK = 0, ST_DEFERRED = 1, ST_OVERFLOW = 2, ST_RETRY = 3,
       ST_DONE = 4,
       ST_OK_ORDERED = 5 };  // ST_OK, and no trim_hits of the spectrum dropped anything: the order-free list IS the reference's list  // reported by the fused narrow kernel: nothing left to do for the per-phase kernels of the same pass
enum { CTR_QUEUED = 0, CTR_LIST_OVERFLOW = 1, CTR_QUEUE_HEAD = 2, CTR_ARENA_PTR = 3, CTR_ARENA_OVERFLOW = 4, CTR_RETRY = 5,
       CTR_TIED = 6,  // narrow spectra whose tie at a reported rank the fused kernel settled in place
       CTR_FAST_TIE = 7,  // (unused since round 6: the stripes below)
       // spectra whose tie at the top rescore_kernel settled from the stored window counts (statistics: SageTiming::n_tied), in
       // CTR_TIE_STRIPES counters 64 bytes apart, a workgroup's by its id: one counter took one atomic per tied spectrum on ONE
       // address — 312 816 per step of the tie-rich C3T, and same-address atomics retire at ~87 M/s: 5.5 % of its rescoring kernel
       CTR_TIE_STRIPE0 = 16, CTR_TIE_STRIPES = 16, CTR_TIE_STRIDE = 16,
       CTR_COUNT = CTR_TIE_STRIPE0 + CTR_TIE_STRIPES * CTR_TIE_STRIDE };

// one precursor-window query (scoring.rs:335-382) of a spectrum handled by the large-window pipeline
struct QueryRec {
    uint32_t left;        // pre_idx_lo: candidate slot s <-> peptide left + s
    uint32_t potential;   // number of candidate slots (scoring.rs:351); 0 == query not evaluated
    uint32_t matched;     // InitialHits.matched_peaks of this query
    uint32_t scored;      // InitialHits.scored_candidates of this query
    uint32_t head;        // the query's candidate directory in the arena (0xFFFFFFFF: none): n_dir entries {position, count}
    uint32_t z_iso;       // precursor charge | (isotope error + 128) << 8
    uint32_t pad[2];      // [0] bit 0: some count >= 63 (clipped histogram), bits 8..: k-th largest count T; [1] slots == T to skip
    uint32_t n_dir;       // directory entries: tiles of the window x wavefronts of the count kernel, in slot order
    uint32_t t0;          // first tile of the window
    uint32_t n_cand;      // candidate words behind the directory (the length of the stream a heap replay walks)
};

// device-side SageFragments (sage_hip.h)
struct DevFragments {
    uint64_t capacity;
    uint8_t* kinds;
    int32_t* charges;
    int32_t* fragment_ordinals;
    float* intensities;
    float* mz_calculated;
    float* mz_experimental;
};

struct TileParams {
    DevDbView db;
    DevScorer sc;
    DevBatchView b;
    DevWork w;
};

// launch wrappers (kernels.hip)
size_t prelim_lds_bytes(const DevScorer& sc, const DevBatchView& b, bool huge = false);
size_t huge_stride_bytes(const DevScorer& sc);  // bytes of DevWork::hugebuf per workgroup of the wide-list kernels
uint32_t huge_grid();
size_t tile_lds_bytes(const DevDbView& db, const DevScorer& sc, const DevBatchView& b, bool cnt8 = false, bool wing = false);
int tile_kernel_prepare(size_t max_lds_bytes);  // raises the kernel's dynamic-LDS limit; returns a hipError_t
int spectrum_kernel_prepare(size_t max_lds_bytes);  // ... of the per-spectrum kernels (spectra of thousands of peaks)
int bigk_kernel_prepare(size_t max_lds_bytes);  // ... of the instances for lists wider than a wavefront (report_psms > 32)
size_t assemble_lds_bytes(const DevScorer& sc);
uint32_t fast_tie_lds_words();  // words of LDS rescore_kernel can stage a spectrum's window counts in ((wcap + 1) / 2 must fit)
size_t rescore_lds_bytes(const DevScorer& sc, const DevBatchView& b, uint32_t max_ions, bool quick, bool huge = false);
size_t narrow_lds_bytes(const DevScorer& sc, const DevBatchView& b);
// the narrow search as ONE launch of two kinds of workgroups (preliminary / rescoring, kernels.hip: search_kernel)
size_t search_lds_bytes(const DevScorer& sc, const DevBatchView& b);
void launch_search(const DevDbView& db, const DevScorer& sc, const DevBatchView& b, const DevWork& w, const double* lnfact_table,
                   uint32_t lnfact_n, SageFeature* out, uint32_t* out_count, void* stream);
// the fused narrow-search kernel: preliminary matching + k-select + rescoring of every spectrum whose windows fit the LDS counters
void launch_narrow(const DevDbView& db, const DevScorer& sc, const DevBatchView& b, const DevWork& w, const double* lnfact_table,
                   uint32_t lnfact_n, SageFeature* out, uint32_t* out_count, void* stream);
void launch_prelim(const DevDbView& db, const DevScorer& sc, const DevBatchView& b, const DevWork& w, void* stream);
void launch_queue(const DevScorer& sc, const DevBatchView& b, const DevWork& w, void* stream);  // (DevWork::queue_later)
// `side`: a second stream + two events (hipStream_t, hipEvent_t x 2) for the launches that may run next to each other, or null
struct SideStream {
    void* stream;
    void* fork;
    void* join;
};
void launch_prelim_tile(const DevDbView& db, const DevScorer& sc, const DevBatchView& b, const DevWork& w, void* stream,
                        const SideStream* side = nullptr);
uint32_t queries_per_spectrum(const DevScorer& sc);
// index_build.hip (each returns a hipError_t)
int generate_fragments_on_device(uint64_t np, uint32_t nk, const uint8_t* d_kinds, const uint64_t* d_seq_off, const uint8_t* d_seq,
                                 const float* d_mods, const float* d_nterm, const float* d_mono, uint64_t min_ion_index,
                                 const uint64_t* d_ion_off, const uint64_t* d_pm_off, float* d_ions, SageTheoretical* d_pm_frag,
                                 void* stream);
int ion_abs_range_on_device(const float* d_ions, uint64_t n, uint32_t* lo_bits, uint32_t* hi_bits);
int rebuild_peptide_major_on_device(const SageTheoretical* d_tm_frag, uint64_t nf, SageTheoretical* d_pm_frag, void* stream);
// (build_tile_copy_on_device, build_succinct_lut_on_device, build_peptide_mass_lut: hip_host.h — they fill owning buffers)
// rescore.hip
int rescore_on_device(int device, const SageRescoreInput& in, SageRescoreOutput& out, std::string& err);
// rt_model.hip
int predict_rt_on_device(int device, const SageRtInput& in, SageRtOutput& out, std::string& err);
// lfq.hip
int lfq_on_device(int device, const SageLfqInput& in, const SageLfqMobility* mobility, SageLfqOutput& out, std::string& err);
// tmt.hip: sage_hip_tmt behind its null-argument checks
int tmt_on_device(int device, const SageTmtInput& in, SageTmtOutput& out, std::string& err);
// protein_lfq.hip: sage_hip_protein_lfq behind its argument checks (n_rows, n_files and n_proteins all non-zero)
int protein_lfq_on_device(int device, const SageProteinLfqInput& in, SageProteinLfqOutput& out, std::string& err);
// purity.hip: sage_hip_precursor_purity behind its argument checks (n_queries non-zero, every array present and in range)
int purity_on_device(int device, const SagePurityInput& in, SagePurityOutput& out, std::string& err);
// tmt_rollup.hip: sage_hip_tmt_rollup behind its argument checks (n_rows, n_labels and n_groups all non-zero, every id in range)
int tmt_rollup_on_device(int device, const SageTmtRollupInput& in, SageTmtRollupOutput& out, std::string& err);
// launch schedule of a batch (index_build.hip): order[k] = spectrum scored by block k, ascending neutral precursor mass
size_t schedule_temp_bytes(uint32_t n);
int schedule_on_device(uint32_t n, const float* d_precursor_mz, const uint8_t* d_charge, uint32_t min_charge, uint32_t* d_keys_a,
                       uint32_t* d_keys_b, uint32_t* d_idx, uint32_t* d_order, void* d_temp, size_t temp_bytes, void* stream);
void schedule_records_on_device(uint32_t n, const uint32_t* d_order, const uint64_t* d_peak_off, const float* d_precursor_mz,
                                const uint8_t* d_charge, const float* d_iso_lo, const float* d_iso_hi, const uint8_t* d_iso_kind,
                                uint4* d_sched, uint32_t stride, void* stream);
// process.hip (process_raw_on_device: hip_host.h)
size_t process_lds_bytes(uint32_t rcap, uint32_t rpow2);
int process_kernel_prepare(size_t max_lds_bytes);
void launch_process(uint32_t n, const uint64_t* raw_off, const float* raw_mz, const float* raw_int, const uint8_t* charge,
                    uint32_t take_top_n, bool deisotope, float min_deisotope_mz, uint32_t rcap, uint32_t rpow2, uint32_t stride,
                    float* out_mass, float* out_int, float* out_tic, uint32_t* out_count, void* stream);
void launch_process_big(uint32_t n_big, const uint32_t* big_list, unsigned char* workspace, const uint64_t* raw_off, const float* raw_mz,
                        const float* raw_int, const uint8_t* charge, uint32_t take_top_n, bool deisotope, float min_deisotope_mz,
                        uint32_t big_cap, uint32_t big_pow2, uint32_t stride, float* out_mass, float* out_int, float* out_tic,
                        uint32_t* out_count, void* stream);
void launch_compact(uint32_t n, const uint64_t* peak_off, uint32_t stride, const float* sm, const float* si, float* masses,
                    float* intens, void* stream);
// DevScorer::rescore_general
constexpr uint32_t RESCORE_GENERAL_CHIMERA = 1u, RESCORE_GENERAL_KINDS = 2u;
// The instance of the rescoring kernels a launch_rescore with these arguments takes (sage_hip_debug_rescore_instance; include/sage_hip.h:
// SAGE_HIP_RESCORE_INST_*): the template arguments of rescore_kernel as bits, or RESCORE_INST_BIG for rescore_big_kernel.
constexpr uint32_t RESCORE_INST_CHIMERA = 1u, RESCORE_INST_KINDS2 = 2u, RESCORE_INST_FAST = 4u, RESCORE_INST_ACC = 8u, RESCORE_INST_PROF = 16u,
                   RESCORE_INST_BIG = 32u, RESCORE_INST_NONE = 0xFFFFFFFFu;
uint32_t rescore_instance_code(const DevScorer& sc, const DevWork& w, bool quick);
// (returns a hipError_t: hipErrorInvalidValue when `keep` would meet an instance compiled without quick_score's block)
int launch_rescore(const DevDbView& db, const DevScorer& sc, const DevBatchView& b, const DevWork& w,
                   const double* lnfact_table, uint32_t lnfact_n, uint32_t max_ions, SageFeature* out,
                   uint32_t* out_count, uint8_t* keep, void* stream);
// counts[n] -> h_counts (device view of page-locked memory) and the counter blocks (2 * CTR_COUNT words) of up to four parts
struct EpilogueParts {
    uint32_t* src[4];  // (reset by the kernel after the copy)
    uint32_t* dst[4];
    uint32_t n;
};
void launch_epilogue(const uint32_t* counts, uint32_t n, uint32_t* h_counts, const uint32_t* order, const EpilogueParts& parts, void* stream);
void launch_window_max(const DevScorer& sc, const DevBatchView& b, const float* pep_mono, uint32_t np, uint32_t* out_max, uint4* win_out,
                       void* stream);
void launch_quick_mark(const DevScorer& sc, const DevBatchView& b, const DevWork& w, uint8_t* keep, void* stream);
void launch_annotate(const DevDbView& db, const DevScorer& sc, const DevBatchView& b, const SageFeature* feats,
                     const uint32_t* counts, const uint64_t* psm_off, const DevFragments& out, void* stream);
// candidates_kernel: score_candidate of the peptides cand_pep[cand_off[slot] ..) for the PSM slots of the n_list spectra of spec_list
size_t candidates_lds_bytes(const DevBatchView& b);
void launch_candidates(const DevDbView& db, const DevScorer& sc, const DevBatchView& b, const SageFeature* feats, const uint32_t* counts,
                       const uint32_t* spec_list, uint32_t n_list, const uint64_t* cand_off, const uint32_t* cand_pep,
                       const uint8_t* cand_charge, const double* lnfact_table, uint32_t lnfact_n, SageCandidateScore* out, void* stream);
// depth_counts_kernel / site_counts_kernel (site localisation): the depth counts of every candidate; the counts over the
// site-determining items of the pair (pair_a[slot], pair_b[slot]: positions in the slot's list, pair_b == 0xFFFFFFFF: no pair)
struct DevSiteCounts {
    uint32_t n_site_items;
    uint32_t a[5], b[5];  // a[1..10], b[1..10] as u16 pairs, the lower depth in the low half
};
size_t localise_lds_bytes(const DevBatchView& b);
void launch_depth_counts(const DevDbView& db, const DevScorer& sc, const DevBatchView& b, const SageFeature* feats, const uint32_t* counts,
                         const uint32_t* spec_list, uint32_t n_list, const uint64_t* cand_off, const uint32_t* cand_pep,
                         const uint8_t* cand_charge, SageDepthCounts* out, void* stream);
void launch_site_counts(const DevDbView& db, const DevScorer& sc, const DevBatchView& b, const SageFeature* feats, const uint32_t* counts,
                        const uint32_t* spec_list, uint32_t n_list, const uint64_t* cand_off, const uint32_t* cand_pep,
                        const uint8_t* cand_charge, const uint32_t* pair_a, const uint32_t* pair_b, DevSiteCounts* out, void* stream);

}  // namespace sagehip
