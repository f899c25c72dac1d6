/*
 * sage_hip.h — C ABI of the MI355X-native search-and-score engine (libsage_hip.so).
 *
 * This is the drop-in boundary for ONE path of lazear/sage: `Scorer::score` /
 * `score_chimera_fast` over `IndexedDatabase` (reference citations are relative to
 * /root/reference/crates/sage/src unless a crate is named).  The reference has no FFI; the entry
 * points below are what a Rust `extern "C"` shim inside sage-core would bind (INTEGRATION.md shows
 * the shim).  Conventions:
 *   - plain pointers and sizes only; the caller owns every input buffer for the duration of a call;
 *     outputs are caller-allocated;
 *   - every function returns a status code (SAGE_HIP_OK == 0) instead of panicking
 *     (the reference panics at scoring.rs:261-267, 301-304, 466-468); sage_hip_last_error() gives
 *     the message of the last failure on the calling thread;
 *   - a SageScorer handle may be shared by any number of host threads, like `&Scorer` (scoring.rs:300 is called from every
 *     rayon worker): calls on ONE handle run one after the other; sage_hip_scorer_clone() gives a thread its own handle
 *     (own streams and working set, same device database) when batches should be scored concurrently.  Use one device
 *     database + scorer per device for multi-GPU (spectra sharded, index replicated, no collective on the data path).
 *   - there is NO CPU fallback: scoring entry points fail with SAGE_HIP_ERR_NO_DEVICE when no
 *     gfx950 device is usable.
 */
#ifndef SAGE_HIP_H
#define SAGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_HIP_ABI_VERSION 6

enum {
    SAGE_HIP_OK = 0,
    SAGE_HIP_ERR_INVALID = 1,     /* bad argument / contract violation (reference: panic!) */
    SAGE_HIP_ERR_NO_DEVICE = 2,   /* no usable HIP device */
    SAGE_HIP_ERR_HIP = 3,         /* a HIP runtime call failed */
    SAGE_HIP_ERR_UNSUPPORTED = 4, /* valid in the reference, outside this build's device limits */
    SAGE_HIP_ERR_OOM = 5,
    SAGE_HIP_ERR_INTERNAL = 6     /* an invariant of the library itself did not hold (a bug: report it) */
};

/* mass.rs:10-16  enum Tolerance { Ppm(f32,f32), Pct(f32,f32), Da(f32,f32) } */
enum { SAGE_TOL_PPM = 0, SAGE_TOL_PCT = 1, SAGE_TOL_DA = 2 };
typedef struct SageTolerance {
    int32_t kind;
    float lo, hi;
} SageTolerance;

/* ion_series.rs:6-15  enum Kind { A, B, C, X, Y, Z } */
enum { SAGE_ION_A = 0, SAGE_ION_B = 1, SAGE_ION_C = 2, SAGE_ION_X = 3, SAGE_ION_Y = 4, SAGE_ION_Z = 5 };

/* database.rs:378-382  struct Theoretical */
typedef struct SageTheoretical {
    uint32_t peptide_index; /* PeptideIx, database.rs:367-369 */
    float fragment_mz;
} SageTheoretical;

/* ------------------------------------------------------------------------------------------
 * Host side: database construction.  Replaces database.rs:59-139 (Builder / Parameters) and
 * Parameters::build (database.rs:260-364).  Option<T> fields use -1 / NULL for None.
 * ---------------------------------------------------------------------------------------- */
typedef struct SageDbParams {
    uint64_t bucket_size;      /* 0 => 8192; rounded up to a power of two (database.rs:97) */
    int32_t missed_cleavages;  /* EnzymeBuilder fields, database.rs:15-27 */
    int32_t min_len, max_len;
    const char* cleave_at;
    const char* restrict_;
    int32_t c_terminal;
    int32_t semi_enzymatic;
    int32_t enzyme_present;    /* 0 => the whole `enzyme` object is absent (database.rs:105) */
    float peptide_min_mass, peptide_max_mass;
    const uint8_t* ion_kinds;  /* SAGE_ION_* ; NULL/0 => [b, y] */
    uint32_t n_ion_kinds;
    uint64_t min_ion_index;
    const char* const* static_mod_keys; /* "C", "^", "$K", "[", ... (modification.rs:66-104) */
    const float* static_mod_masses;
    uint32_t n_static_mods;
    const char* const* var_mod_keys;    /* one entry per (key, mass) pair */
    const float* var_mod_masses;
    uint32_t n_var_mods;
    uint64_t max_variable_mods;
    const char* decoy_tag;
    int32_t generate_decoys;
    int32_t peptides_only;     /* 1 => stop after reorder_peptides (database.rs:221-258): no fragments / min_value; the index is
                                  then generated on the device by sage_hip_db_create (build_from_peptides, :265-346) */
} SageDbParams;

/* Flat, read-only view of an IndexedDatabase (database.rs:384-395) + the Peptide fields the path
 * reads (peptide.rs:12-31).  nterm/cterm: NaN == None. */
typedef struct SageDbView {
    const SageTheoretical* fragments; /* globally m/z sorted, then peptide-sorted inside each bucket */
    uint64_t n_fragments;
    const float* min_value;           /* [n_buckets] */
    uint64_t n_buckets;
    uint64_t bucket_size;
    const float* pep_mono;            /* [n_peptides], ascending (total_cmp) */
    const uint64_t* seq_off;          /* [n_peptides + 1] */
    const uint8_t* seq;               /* residues, ASCII */
    const float* mods;                /* per-residue modification mass, parallel to seq */
    const float* nterm;
    const float* cterm;
    const uint8_t* decoy;
    const uint8_t* missed_cleavages;
    uint64_t n_peptides;
    const uint8_t* ion_kinds;
    uint32_t n_ion_kinds;
    uint64_t min_ion_index;           /* read only when fragments == NULL (device-side build_from_peptides) */
} SageDbView;

typedef struct SageHostDb SageHostDb;

/* Parameters::build(Fasta::parse(text)) — database.rs:260-263, fasta.rs:16-56 */
int sage_hip_hostdb_build(const char* fasta_text, const SageDbParams* params, SageHostDb** out);
/* ---- the `prefilter` flow of sage-cli (runner.rs:104-127, :143-238) ----------------------------------------------------
 * database.prefilter: the FASTA is searched in chunks of `prefilter_chunk_size` target proteins with Scorer::quick_score
 * (sage_hip_quick_score_resident), and the final database holds only the peptides some spectrum picked. */
/* Fasta::parse(..).targets.len() (fasta.rs:16-56) */
int sage_hip_fasta_num_targets(const char* fasta_text, const SageDbParams* params, uint64_t* out);
/* Parameters::auto_calculate_prefilter_chunk_size (database.rs:142-160); `requested` = the configured value, 0 = auto */
int sage_hip_prefilter_chunk_size(const char* fasta_text, const SageDbParams* params, uint64_t requested, uint64_t* out);
/* Parameters::build over targets [first_target, first_target + n_targets): one chunk of Fasta::iter_chunks (fasta.rs:81-89) */
int sage_hip_hostdb_build_chunk(const char* fasta_text, const SageDbParams* params, uint64_t first_target, uint64_t n_targets,
                                SageHostDb** out);
/* runner.rs:215-238: the kept peptides of every chunk (keep[c][ix] != 0, consecutive chunks in FASTA order), through
 * Parameters::reorder_peptides and build_from_peptides (honours params->peptides_only) */
int sage_hip_hostdb_merge_kept(const SageHostDb* const* chunks, const uint8_t* const* keep, uint32_t n_chunks,
                               const SageDbParams* params, SageHostDb** out);
void sage_hip_hostdb_free(SageHostDb* db);
int sage_hip_hostdb_view(const SageHostDb* db, SageDbView* out);
/* Display string of peptide i ("[+42]-MEWK...", peptide.rs:391-408) and its ';'-joined proteins;
 * return the required buffer size including NUL. */
uint64_t sage_hip_hostdb_peptide_string(const SageHostDb* db, uint64_t i, char* out, uint64_t cap);
uint64_t sage_hip_hostdb_peptide_proteins(const SageHostDb* db, uint64_t i, char* out, uint64_t cap);
/* Peptide.proteins.len() and Peptide.semi_enzymatic (peptide.rs:28-30) — columns of results.sage.tsv */
int sage_hip_hostdb_peptide_info(const SageHostDb* db, uint64_t i, uint32_t* num_proteins, uint8_t* semi_enzymatic);

/* SpectrumProcessor::new(take_top_n, deisotope, min_deisotope_mz).process() for one centroided
 * MS2 spectrum (spectrum.rs:279-412).  precursor_charge 0 == None.  out_* need capacity n.
 * Returns the number of peaks kept. */
uint64_t sage_hip_process_ms2(uint64_t take_top_n, int deisotope, float min_deisotope_mz, const float* mz,
                              const float* intensity, uint64_t n, uint8_t precursor_charge, float* out_mass,
                              float* out_intensity, float* out_tic);

/* ------------------------------------------------------------------------------------------
 * Device side.
 * ---------------------------------------------------------------------------------------- */
typedef struct SageDeviceDb SageDeviceDb;
typedef struct SageScorer SageScorer;
typedef struct SageDeviceBatch SageDeviceBatch;

int sage_hip_device_count(void);

/* Upload an IndexedDatabase to HBM on `device` and derive the device layouts.
 * Stands in for the `&'db IndexedDatabase` borrow of Scorer (scoring.rs:211).
 * With view->fragments == NULL the fragment index is generated ON THE DEVICE from the peptide list
 * (Parameters::build_from_peptides, database.rs:265-346: ion series, stored-ion filter by view->min_ion_index, sort).
 * Peptides of any length up to 65 535 residues (beyond 1023 the general, slower rescoring instance scores the database: DESIGN.md 4.8;
 * the reference's default max_len is 50). */
int sage_hip_db_create(const SageDbView* view, int device, SageDeviceDb** out);
void sage_hip_db_destroy(SageDeviceDb* db);
uint64_t sage_hip_db_device_bytes(const SageDeviceDb* db);

/* scoring.rs:210-232  struct Scorer — every field, same meaning. */
typedef struct SageScorerParams {
    SageTolerance precursor_tol, fragment_tol;
    uint16_t min_matched_peaks;
    int8_t min_isotope_err, max_isotope_err;
    uint8_t min_precursor_charge, max_precursor_charge;
    uint8_t override_precursor_charge;
    uint8_t chimera;
    int16_t max_fragment_charge; /* Option<u8>: -1 == None */
    uint8_t wide_window;
    uint8_t annotate_matches;    /* the Fragments themselves are fetched with sage_hip_annotate_resident */
    uint32_t report_psms;        /* 1..32767 (above 32: the wider, slower kernels of DESIGN.md 4.8; lists that do not fit a compute unit's
                                  * LDS live in a global-memory workspace) */
    int32_t score_type;          /* 0 SageHyperScore, 1 OpenMSHyperScore (scoring.rs:10-14) */
} SageScorerParams;

int sage_hip_scorer_create(SageDeviceDb* db, const SageScorerParams* params, SageScorer** out);
/* A second handle with the same parameters on the same device database (`&Scorer` is Sync: runner.rs:311-325 calls score from
 * every worker thread).  Handles are independent: own streams, own device working set. */
int sage_hip_scorer_clone(SageScorer* scorer, SageScorer** out);
void sage_hip_scorer_destroy(SageScorer* scorer);

/* A batch of ProcessedSpectrum (spectrum.rs:57-79) + precursors[0] (spectrum.rs:46-55), SoA.
 * All spectra must be MS2 (level == 2 is asserted by the reference at scoring.rs:301-304). */
typedef struct SageSpectrumBatch {
    uint32_t n_spectra;
    const uint64_t* peak_off;          /* [n + 1] */
    const float* masses;               /* ascending inside each spectrum */
    const float* intensities;
    const float* precursor_mz;         /* [n] precursors[0].mz */
    const uint8_t* precursor_charge;   /* [n] 0 == None */
    const float* isolation_lo;         /* [n] isolation_window = Tolerance::Da(lo, hi); NaN == None; may be NULL */
    const float* isolation_hi;
    const float* total_ion_current;    /* [n] */
    const float* scan_start_time;      /* [n] may be NULL (0) */
    const float* inverse_ion_mobility; /* [n] NaN == None; may be NULL */
    const uint32_t* file_id;           /* [n] may be NULL (0) */
} SageSpectrumBatch;

/* scoring.rs:69-149  struct Feature — the fields the hot path computes (the rest are defaults the
 * reference fills in later, scoring.rs:576-592).  psm_id (a global atomic, :163-167) is excluded. */
typedef struct SageFeature {
    uint32_t spec_index; /* position in the batch; stands in for spec_id */
    uint32_t peptide_idx;
    uint32_t rank;
    int32_t label;
    float expmass, calcmass, rt, ims, delta_mass, isotope_error, average_ppm;
    float longest_y_pct, matched_intensity_pct, ms2_intensity;
    double hyperscore, delta_next, delta_best, poisson;
    uint32_t matched_peaks, longest_b, longest_y, scored_candidates;
    uint32_t peptide_len, file_id;
    uint8_t charge, missed_cleavages;
    uint8_t pad[6];
} SageFeature;

/* Scorer::score for every spectrum of the batch (scoring.rs:300-309), results in input order:
 * out[i*report_psms + r] for r < out_count[i], Feature.spec_index == i.
 * Host memory in, host memory out, as a pipeline over chunks of the batch (SAGE_HIP_CHUNK spectra, default 131072): the
 * uploads run up to three chunks ahead on a copy stream while earlier chunks are scored (two at a time when the batch has no
 * large precursor windows) and their PSM records come back — the reader / processor / search overlap of runner.rs:365-375,
 * 450-461 at the PCIe boundary.  Arrays allocated with
 * sage_hip_host_alloc (page-locked) move by DMA at full PCIe rate; pageable arrays are accepted and staged through
 * page-locked blocks by a few host threads.  A chunk whose large-window candidates exhaust the device arena is scored again
 * in halves (never an error unless a single spectrum does not fit). */
int sage_hip_score_batch(SageScorer* scorer, const SageSpectrumBatch* batch, SageFeature* out,
                         uint32_t* out_count);

/* The same split in two so a batch can stay resident in HBM across calls.  `out` allocated with sage_hip_host_alloc
 * (page-locked, mapped) is written by the rescoring kernels themselves — no download phase; it holds the results when the
 * call returns.  Any other host memory gets a device buffer and a copy. */
int sage_hip_batch_upload(SageScorer* scorer, const SageSpectrumBatch* batch, SageDeviceBatch** out);
void sage_hip_batch_free(SageDeviceBatch* batch);
int sage_hip_score_resident(SageScorer* scorer, SageDeviceBatch* batch, SageFeature* out, uint32_t* out_count);

/* Raw centroided MS2 spectra (spectrum.rs:81-106 RawSpectrum + precursors[0]), SoA — the input of
 * SpectrumProcessor::process.  Same conventions as SageSpectrumBatch; peaks in any order (MGF keeps the file's order): like the
 * reference (spectrum.rs:179-227, 279-335), preprocessing uses them as given, without sorting first. */
typedef struct SageRawBatch {
    uint32_t n_spectra;
    const uint64_t* peak_off;          /* [n + 1] */
    const float* mz;
    const float* intensities;
    const float* precursor_mz;         /* [n] */
    const uint8_t* precursor_charge;   /* [n] 0 == None (then fragments are deisotoped up to z = 3, spectrum.rs:289-293) */
    const float* isolation_lo;         /* [n] may be NULL */
    const float* isolation_hi;
    const float* scan_start_time;      /* [n] may be NULL */
    const float* inverse_ion_mobility; /* [n] may be NULL */
    const uint32_t* file_id;           /* [n] may be NULL */
} SageRawBatch;

/* SpectrumProcessor::new(take_top_n, deisotope, min_deisotope_mz).process() (spectrum.rs:279-412) for every spectrum of
 * the batch ON THE DEVICE, leaving the ProcessedSpectrum arrays resident for sage_hip_score_resident: raw peaks in, PSMs
 * out, no host round trip in between.  Spectra that keep fewer than `min_peaks` peaks are not searched (sage-cli
 * runner.rs:313): they stay in the batch with zero peaks and yield no PSM.  out_npeaks (optional, [n]) receives the
 * number of peaks each spectrum kept before that filter. */
int sage_hip_batch_process_upload(SageScorer* scorer, const SageRawBatch* raw, uint64_t take_top_n, int deisotope,
                                  float min_deisotope_mz, uint32_t min_peaks, SageDeviceBatch** out, uint32_t* out_npeaks);
/* Copy a resident batch's ProcessedSpectrum arrays back (tests, writers).  peak_off: [n + 1]; masses / intensities need
 * peak_off[n] entries — call once with masses == NULL to get peak_off first. */
int sage_hip_batch_download(SageDeviceBatch* batch, uint64_t* peak_off, float* masses, float* intensities, float* tic);

/* Scorer::initial_hits (scoring.rs:418-462) of every spectrum of a resident batch: the trimmed
 * preliminary list in the reference's heap-layout order.  packed[i*cap + j] =
 * matched<<48 | peptide<<16 | precursor_charge<<8 | (isotope_error+128); len[i] entries are valid. */
int sage_hip_initial_hits(SageScorer* scorer, SageDeviceBatch* batch, uint64_t* packed, uint32_t cap,
                          uint32_t* len, uint64_t* matched_peaks, uint64_t* scored_candidates);

/* scoring.rs:152-161  struct Fragments of every reported PSM (Scorer.annotate_matches, scoring.rs:722-752), flattened:
 * PSM r of spectrum i is slot s = i * report_psms + r and owns entries [psm_off[s], psm_off[s + 1]) of each array, in the
 * reference's push order (ion kind, ion index, fragment charge).  A slot's length equals its Feature.matched_peaks, so the
 * caller can size the arrays from the features; `capacity` is the number of entries available in each array. */
typedef struct SageFragments {
    uint64_t capacity;
    uint64_t* psm_off;            /* [n_spectra * report_psms + 1] */
    uint8_t* kinds;               /* SAGE_ION_* */
    int32_t* charges;
    int32_t* fragment_ordinals;
    float* intensities;
    float* mz_calculated;
    float* mz_experimental;
} SageFragments;
/* Annotate the PSMs `features` / `counts` that sage_hip_score_resident returned for this resident batch with this scorer
 * (with chimera, the winner's peaks are removed between PSMs exactly as score_chimera_fast does).  Fails with
 * SAGE_HIP_ERR_INVALID when `capacity` is too small; out->psm_off is filled either way. */
int sage_hip_annotate_resident(SageScorer* scorer, SageDeviceBatch* batch, const SageFeature* features,
                               const uint32_t* counts, SageFragments* out);

/* Scorer::quick_score (scoring.rs:255-298) for every spectrum of a resident batch — the first pass of the `prefilter`
 * flow (sage-cli runner.rs:143-240).  keep: host array [n_peptides] standing in for the reference's &[AtomicBool];
 * identified peptides are OR-ed in (keep[i] = 1). */
int sage_hip_quick_score_resident(SageScorer* scorer, SageDeviceBatch* batch, int prefilter_low_memory, uint8_t* keep);

/* Timing of the last sage_hip_score_resident / sage_hip_score_batch call, from HIP events recorded
 * on the scorer's own stream. */
typedef struct SageTiming {
    float prelim_ms;   /* fragment-match + k-select kernel(s) */
    float rescore_ms;  /* rescoring + top-K + Feature kernel */
    float total_ms;    /* first launch -> last kernel done (excludes H2D/D2H) */
    uint32_t n_launches;
    uint32_t n_wide;   /* spectra routed to the tiled large-window kernels */
    uint32_t arena_entries; /* 4-byte entries of the large-window candidate arena this call used */
    uint32_t n_retry;  /* spectra with equal hyperscores at a reported rank, re-run with exact heap layouts (the retry pass) */
    float retry_ms;    /* of total_ms: that retry pass */
    uint32_t n_tied;   /* SAGE_HIP_FUSED=1 only: narrow spectra with such a tie, settled inside the fused first-pass kernel */
    uint32_t n_ways;   /* sage_hip_score_resident: parts of the batch scored next to each other on their own streams (then
                        * prelim_ms / rescore_ms are sums over parts that overlap in time; total_ms is the wall span) */
} SageTiming;
int sage_hip_last_timing(const SageScorer* scorer, SageTiming* out);
/* The per-kernel times of SageTiming (prelim_ms / rescore_ms / retry_ms / total_ms) come from HIP events recorded between the
 * kernels of a sage_hip_score_resident call: eight records and six elapsed-time queries, ~15 us of a call — nothing next to a
 * 500 000-spectrum step, 2 % of a 62 500-spectrum one.  `every` = 1 (the default): every call is timed; n > 1: every n-th call,
 * the calls in between report the kernel times of the last timed call and total_ms == 0; 0: never.  The counters (n_retry, n_wide,
 * ...) are always the call's own.  No counterpart in the reference (runner.rs:327-330 times the whole search with a wall clock). */
int sage_hip_scorer_set_timing_interval(SageScorer* scorer, uint32_t every);

/* Page-locked host memory for `out` / `out_count`: results then arrive by DMA at full PCIe rate instead of
 * through the runtime's staging copy.  Optional — any host pointer is accepted by the scoring calls. */
int sage_hip_host_alloc(uint64_t bytes, void** out);
void sage_hip_host_free(void* p);

/* Debug aid, only with SAGE_HIP_PHASE_CLOCKS=1 at scorer creation: cumulative shader cycles per kernel phase over the
 * first 4096 work items, out32[8*k + phase]: k = 0 narrow preliminary kernel, 1 rescoring kernel, 2 large-window count
 * kernel, 3 large-window replay kernel. */
int sage_hip_debug_phase_cycles(SageScorer* scorer, unsigned long long* out32);
/* Debug aid, same condition: what the rescoring kernels' prune dropped since the scorer was created. out4[0] candidates that could
 * not reach min_matched_peaks any more, [1] their (ion, fragment charge) items, [2] scoring rounds that ended before the
 * hyperscore because no candidate reached it, [3] rounds in which a passing candidate stood beside pruned ones. */
int sage_hip_debug_prune_counters(SageScorer* scorer, unsigned long long* out4);
/* Debug aid, same condition: the trips of the rescoring kernels' peak-bitmap filter since the scorer was created. out4[0] 64-ion
 * chunks that took the flat route (ions dealt to all lanes), [1] their trips of 8 ions, [2] the trips of 4 ions the per-lane
 * filter would have made of those chunks, [3] the trips of 4 ions of the chunks that took the per-lane route. */
int sage_hip_debug_filter_counters(SageScorer* scorer, unsigned long long* out4);
/* Debug aid, same condition: the cooperative path of the rescoring kernels (a candidate with many hits in a 64-ion chunk is matched
 * by the whole wavefront) since the scorer was created. out2[0] chunks of candidates taken that way, [1] the (ion, fragment charge)
 * matches added up for them. */
int sage_hip_debug_heavy_counters(SageScorer* scorer, unsigned long long* out2);
/* Debug aid, same condition: the route those chunks took. out2[0] chunks whose (ion, fragment charge) items went through one lookup
 * trip, one item per lane, with the three sums made from LDS, [1] chunks that took a trip per fragment charge and the sums by
 * readlane (more than 64 items, not the candidate's last chunk, a kernel instance without the route, or
 * SAGE_HIP_DEBUG_FLAGS=262144 at scorer creation, which forces it). */
int sage_hip_debug_heavy_routes(SageScorer* scorer, unsigned long long* out2);
/* Debug aid (no condition): *out = 1 if the first pass of the scorer's last scoring step handed its preliminary lists to the
 * rescoring kernel in rows by schedule position, 0 if in the arrays indexed by spectrum (SAGE_HIP_DEBUG_FLAGS=131072 at scorer
 * creation forces the latter; so does every step that is not the plain narrow search with schedule records). */
int sage_hip_debug_handover_route(SageScorer* scorer, uint32_t* out);
/* Debug aid (no condition): *out = the instance of the rescoring kernel the first pass of the scorer's last scoring step (or its last
 * quick_score) launched, as bits: CHIMERA the general instance with chimera rounds (a chimera search, or SAGE_HIP_RESCORE_GENERAL=1
 * at scorer creation); KINDS2 the instance compiled for a database of exactly two ion kinds, the first n-terminal (a / b / c) and
 * the second not — {b, y}, {c, z}, {a, x} — taken by searches without chimera rounds unless SAGE_HIP_RESCORE_KINDS_GENERAL=1 at
 * scorer creation; FAST the short divisions; ACC the full logarithm and quick_score; PROF the phase clocks (SAGE_HIP_PHASE_CLOCKS=1).
 * BIG: the kernel for lists wider than a wavefront instead (report_psms > 32, peptides beyond 1023 residues).  NONE: no launch yet. */
#define SAGE_HIP_RESCORE_INST_CHIMERA 1u
#define SAGE_HIP_RESCORE_INST_KINDS2 2u
#define SAGE_HIP_RESCORE_INST_FAST 4u
#define SAGE_HIP_RESCORE_INST_ACC 8u
#define SAGE_HIP_RESCORE_INST_PROF 16u
#define SAGE_HIP_RESCORE_INST_BIG 32u
#define SAGE_HIP_RESCORE_INST_NONE 0xFFFFFFFFu
int sage_hip_debug_rescore_instance(SageScorer* scorer, uint32_t* out);

/* Debug aid (no condition): the device database read back, so that tests can hold every table sage_hip_db_create derived
 *  to a plain restatement, entry for entry.  The layout: the scalars the kernels address the tables with. */
typedef struct SageDbLayout {
    uint64_t np, nf;                 /* peptides; stored fragment entries (without the two padding entries of a copy) */
    uint32_t tile_shift, n_tiles, lut_stride;
    float lut_scale;
    uint32_t tile2_shift, n_tiles2, lut2_stride;
    float lut2_scale;
    uint32_t lut2_words;
    uint32_t pep_lut_bins;           /* 0: no peptide-mass table */
    float pep_lut_inv_w;
    uint32_t ion_lo_bits, ion_hi_bits; /* smallest / largest |ion| of the ion table as f32 bits (none: 0xFFFFFFFF, 0) */
    uint32_t max_ions, max_len;
    uint64_t tm2_pos_len;            /* elements of SAGE_DB_TM2_POS */
} SageDbLayout;
int sage_hip_debug_db_layout(SageDeviceDb* db, SageDbLayout* out);
/* The tables: IONS f32 [ion_off[np]] (without the 8 floats of padding), ION_OFF / PM_OFF u64 [np + 1], PEP_INFO u32 [np], PEP_MONO f32
 * [np], PEP_LUT u32 [pep_lut_bins + 1] (none: size 0), PM_FRAG / TM_FRAG / TM2_FRAG SageTheoretical [nf + 2] (the two padding
 * entries included; PM_FRAG is made from the large-tile copy first if the build released it, and is the [nf] list as generated when
 * SAGE_HIP_KEEP_PM_FRAG was set at creation), TM_LUT u32 [n_tiles * lut_stride], TM2_L1 {u32 bits, u32 rank} [n_tiles2 *
 * lut2_words], TM2_POS u32 [tm2_pos_len]. */
enum {
    SAGE_DB_IONS = 0, SAGE_DB_ION_OFF = 1, SAGE_DB_PM_OFF = 2, SAGE_DB_PEP_INFO = 3, SAGE_DB_PEP_MONO = 4, SAGE_DB_PEP_LUT = 5,
    SAGE_DB_PM_FRAG = 6, SAGE_DB_TM_FRAG = 7, SAGE_DB_TM2_FRAG = 8, SAGE_DB_TM_LUT = 9, SAGE_DB_TM2_L1 = 10, SAGE_DB_TM2_POS = 11
};
/* Copy table `table` to `out` (capacity `cap_bytes`); *out_bytes = the table's size.  out == NULL: the size only.  A table that
 * does not exist: size 0, SAGE_HIP_OK.  An unknown id or a buffer smaller than the table: SAGE_HIP_ERR_INVALID. */
int sage_hip_debug_db_table(SageDeviceDb* db, int table, void* out, uint64_t cap_bytes, uint64_t* out_bytes);

/* ---- post-search rescoring --------------------------------------------------------------
 * The step that consumes the Feature records of ALL searched files (sage-cli runner.rs:536-541):
 *   spectrum_fdr  (runner.rs:281-292)  = ml::linear_discriminant::score_psms (linear_discriminant.rs:133-231: mass-error KDE,
 *                                        20-feature LDA, Gauss-Jordan solve, projection, KDE posterior error) or the heuristic
 *                                        fall-back, then the sort by discriminant and ml::qvalue::spectrum_q_value (qvalue.rs:8-36)
 *   fdr::picked_peptide / picked_protein (fdr.rs:123-187) = Competition::assign_q_value (fdr.rs:60-120)
 * Row-parallel work (feature rows, class sums, scatter matrices, projection, kernel-density sums, sorts, scans) runs on the
 * device; the 20x20 solve and the bandwidth scalars are host arithmetic.  Retention-time / ion-mobility models
 * (ml/retention_model.rs, mobility_model.rs) are not part of this call: their outputs enter through the optional arrays. */
typedef struct SageRescoreInput {
    uint64_t n;                    /* Features of the whole run */
    const SageFeature* features;   /* host, [n] */
    const float* aligned_rt;       /* [n] or NULL: features[i].rt (Feature default, scoring.rs:576-592) */
    const float* delta_rt_model;   /* [n] or NULL: 0.999 */
    const float* delta_ims_model;  /* [n] or NULL: 0.999 */
    SageTolerance precursor_tol;   /* Ppm or Da (Pct is unreachable in the reference, linear_discriminant.rs:142) */
    /* picked competitions: dense ids 0..n_keys-1 (every id used at least once) of the map key the reference builds —
     * peptide: the sequence string, reversed for generated decoys (fdr.rs:126-132); protein: the proteins vector, only for
     * peptides with exactly one protein (fdr.rs:158-160), 0xFFFFFFFF otherwise (protein_q stays 1.0).
     * sage_hip_hostdb_competition_keys() produces both. */
    const uint32_t* peptide_key;   /* [n] */
    uint32_t n_peptide_keys;
    const uint32_t* protein_key;   /* [n] */
    uint32_t n_protein_keys;
} SageRescoreInput;

typedef struct SageRescoreOutput {
    /* caller-allocated host arrays [n], INPUT order */
    float* discriminant_score;
    float* posterior_error;        /* log10 PEP; 1.0 (the Feature default) when the linear model could not be fitted */
    float* spectrum_q;
    float* peptide_q;
    float* protein_q;
    uint32_t* order;               /* [n] or NULL: order[j] = input index of the j-th best PSM — the order the reference
                                      leaves `features` in (runner.rs:290) and writes them out */
    /* filled by the call */
    uint64_t passing_spectrum;     /* PSMs with q <= 0.01 (targets and decoys, qvalue.rs:31) */
    uint64_t passing_peptide;      /* target peptides at 1 % (fdr.rs:105) */
    uint64_t passing_protein;
    int32_t lda_fitted;            /* 0: heuristic discriminant of runner.rs:285-288 */
    double coef[20];               /* LDA coefficients, FEATURE_NAMES order (linear_discriminant.rs:20-41) */
    float device_ms;               /* HIP-event time of all kernels of the call */
} SageRescoreOutput;

int sage_hip_rescore(int device, const SageRescoreInput* in, SageRescoreOutput* out);

/* ---- the predict_rt block of sage-cli (runner.rs:513-530), the producer of SageRescoreInput's optional arrays ----------
 *   features.par_sort_unstable_by(poisson) + spectrum_q_value  (runner.rs:517-520, qvalue.rs:8-36): the training filter
 *   ml::retention_alignment::global_alignment                  (retention_alignment.rs:100-173)  -> aligned_rt
 *   ml::retention_model::predict                               (retention_model.rs:14-90, regression.rs:58-122)
 *   ml::mobility_model::predict                                (mobility_model.rs:14-186)
 * Peptide data the two models embed comes per Feature: sequence bytes and monoisotopic mass of db[features[i].peptide_idx]
 * (sage_hip_hostdb_feature_peptides gathers them). */
typedef struct SageRtInput {
    uint64_t n;
    const SageFeature* features;   /* host, [n]: rt, ims, charge, label, file_id, poisson, peptide_idx are read */
    uint32_t n_files;
    const uint64_t* seq_off;       /* [n + 1] */
    const uint8_t* seq;            /* residues, 'A'..'Z' */
    const float* monoisotopic;     /* [n] */
} SageRtInput;

typedef struct SageAlignment {     /* retention_alignment.rs:92-98 */
    uint32_t file_id;
    float max_rt, slope, intercept;
} SageAlignment;

typedef struct SageRtOutput {
    /* caller-allocated host arrays [n], input order; Feature defaults (scoring.rs:576-592) where a model is not fitted */
    float* spectrum_q;             /* q-values of the poisson-sorted pass */
    float* aligned_rt;
    float* predicted_rt;
    float* delta_rt_model;
    float* predicted_ims;
    float* delta_ims_model;
    SageAlignment* alignments;     /* [n_files] */
    /* filled by the call */
    int32_t rt_fitted, ims_fitted; /* LinearRegression::fit returned Some */
    double rt_r2, ims_r2;
    float device_ms;
} SageRtOutput;

int sage_hip_predict_rt(int device, const SageRtInput* in, SageRtOutput* out);

/* Peptide.sequence / .monoisotopic of db[peptide_idx[i]] for SageRtInput.  Call with seq == NULL to size: seq_off is filled. */
int sage_hip_hostdb_feature_peptides(const SageHostDb* db, const uint32_t* peptide_idx, uint64_t n, uint64_t* seq_off,
                                     uint8_t* seq, float* monoisotopic);

/* ---- mzML input (host; sage-cloudpath/src/mzml.rs:109-403 MzMLReader::with_file_id_and_level_filter(..).parse): the MSn
 * spectra of one file as a SageRawBatch whose arrays the handle owns, ready for sage_hip_batch_process_upload.  ms_level < 0
 * keeps every level.  spectrum ids: sage_hip_mzml_spectrum_id. */
typedef struct SageMzml SageMzml;
int sage_hip_mzml_read(const char* path, uint32_t file_id, int ms_level, SageMzml** out);
/* The inputs the reference refuses to search — it panics while PROCESSING them, the reader accepts them: an MS2 spectrum in
 * profile mode (spectrum.rs:280-286; Representation defaults to Profile, so the centroid term MS:1000127 must be present) or
 * without a precursor (scoring.rs:466-468).  SAGE_HIP_ERR_INVALID with the reference's message; call before searching a run. */
int sage_hip_mzml_check_searchable(const SageMzml* run);
int sage_hip_mzml_view(const SageMzml* run, SageRawBatch* out);
const char* sage_hip_mzml_spectrum_id(const SageMzml* run, uint64_t i);
void sage_hip_mzml_free(SageMzml* run);
/* sage_hip_mzml_read with MzMLReader::set_signal_to_noise(Some(sn_level)) (mzml.rs:371-381): every kept spectrum of MS level
 * sn_level that carries a noise array (MS:1002744) gets intensity[i] /= noise[i], i below the shorter length.  Only a
 * spectrum's own noise array divides it.  sn_level < 0: sage_hip_mzml_read. */
int sage_hip_mzml_read_sn(const char* path, uint32_t file_id, int ms_level, int sn_level, SageMzml** out);
/* RawSpectrum.ion_injection_time (MS:1000927; 0 when absent) and precursors.first().spectrum_ref ("" when absent) */
float sage_hip_mzml_ion_injection_time(const SageMzml* run, uint64_t i);
const char* sage_hip_mzml_precursor_ref(const SageMzml* run, uint64_t i);
/* RawSpectrum.mobility of the MS1 spectra of a run: the per-peak ion-mobility array that converters of timsTOF data write as a
 * third binaryDataArray.  An ADDITION over the reference's mzML reader, which ignores the array (its MS1 mobilities come from the
 * Bruker reader only).  An array is the mobility array when it carries MS:1002893, MS:1002816, MS:1003006, MS:1003007 or
 * MS:1003008 and is neither m/z, intensity nor noise (MS:1002744); 32/64-bit, zlib or not, stored as f32.  It is kept for spectra
 * whose ms level is 1 only (spectrum.rs:344); a length other than the m/z array's fails the read (SAGE_HIP_ERR_INVALID).
 *   _mobility       the column, indexed like SageRawBatch.mz ([peak_off[n]]; 0 inside spectra without the array), or NULL when no
 *                   kept spectrum has one (always NULL for MGF runs); owned by the handle
 *   _has_mobility   out[n]: 1 where RawSpectrum.mobility is Some */
const float* sage_hip_mzml_mobility(const SageMzml* run);
int sage_hip_mzml_has_mobility(const SageMzml* run, uint8_t* out);

/* ---- MGF input (host; sage-cloudpath/src/mgf.rs:325-369 MgfReader::with_file_id(file_id).parse, util.rs:107-118 read_mgf):
 * every spectrum of a .mgf / .mgf.gz file as a SageMzml run (MS2, centroided, no ion mobility, injection time 0, no spectrumRef),
 * read through sage_hip_mzml_view / _spectrum_id / _free.  The reference's rules, quirks included:
 *   - the file-level TOL= / TOLU= / CHARGE= (before the first BEGIN IONS, :333-352) apply from the SECOND spectrum on: only the
 *     init() at END IONS copies them in (:55-70, :316); state is reset only at END IONS, so lines between END IONS and the next
 *     BEGIN IONS belong to the next spectrum (:185-196);
 *   - peak lines (:276-299): unparsable m/z adds nothing, a missing intensity is 1.0, an unparsable one drops the spectrum;
 *   - PEPMASS= (:198-221): first token the m/z (no token: 0; unparsable: no precursor); CHARGE= (:223-236): one charge per ASCII
 *     digit; precursors[0] is the first PEPMASS with the first charge (:86-104);
 *   - isolation window Da(-|TOL|, |TOL|) or Ppm(-|TOL|, |TOL|) for TOLU exactly `Da` / `ppm`, else None (:72-83) — the kind
 *     is sage_hip_mzml_isolation_kinds; RTINSECONDS / 60 (:238-247); TITLE= is the spectrum id (:249-255);
 *     TOL=NaN gives the bounds (+inf, -inf): an empty window, as the reference's NaN bounds match nothing, where NaN would read as None;
 *   - check_spectrum (:115-128) drops spectra with an empty id, no precursor, no peaks or peak arrays of different lengths
 *     (a message on stderr; the rest of the file is read);
 *   - a file without BEGIN IONS (the reference panics), a missing file or text that is not UTF-8: SAGE_HIP_ERR_INVALID.
 * Parsed in parallel pieces cut behind END IONS lines (SAGE_HIP_MGF_PIECE_KB, default 4096); spectra in file order. */
int sage_hip_mgf_read(const char* path, uint32_t file_id, SageMzml** out);
/* out[n]: the SAGE_TOL_* kind of each spectrum's isolation_lo / hi (mzML runs: SAGE_TOL_DA throughout) */
int sage_hip_mzml_isolation_kinds(const SageMzml* run, uint8_t* out);
/* out[n]: 1 where precursors[0].charge is Some(0) (MGF `CHARGE=0`), which SageRawBatch.precursor_charge == 0 cannot tell from
 * None.  The reference then searches around mass 0 in a narrow search and reports no PSM (scoring.rs:439-443). */
int sage_hip_mzml_charge_zero(const SageMzml* run, uint8_t* out);
/* The upload and score entry points with the KIND of every spectrum's isolation window (mgf.rs:72-83: `TOLU=ppm` gives
 * Tolerance::Ppm), which the isolation_lo / isolation_hi of SageSpectrumBatch / SageRawBatch do not carry: iso_kind[n] holds
 * SAGE_TOL_PPM, SAGE_TOL_PCT or SAGE_TOL_DA (NULL: every window Da — exactly the entry points without `_kinds`).  Only the
 * wide-window search reads the windows: `isolation_window * charge` (scoring.rs:427-431, mass.rs:47-57) for every kind. */
int sage_hip_batch_upload_kinds(SageScorer* scorer, const SageSpectrumBatch* batch, const uint8_t* iso_kind, SageDeviceBatch** out);
int sage_hip_batch_process_upload_kinds(SageScorer* scorer, const SageRawBatch* raw, const uint8_t* iso_kind, uint64_t take_top_n,
                                        int deisotope, float min_deisotope_mz, uint32_t min_peaks, SageDeviceBatch** out,
                                        uint32_t* out_npeaks);
int sage_hip_score_batch_kinds(SageScorer* scorer, const SageSpectrumBatch* batch, const uint8_t* iso_kind, SageFeature* out,
                               uint32_t* out_count);
/* str::parse::<f32>() as the MGF reader applies it to `len` bytes at `token`: SAGE_HIP_OK and *out, or SAGE_HIP_ERR_INVALID */
int sage_hip_parse_f32(const char* token, uint64_t len, float* out);

/* ---- writers (host): results.sage.tsv / results.sage.pin, byte for byte as sage-cli/src/runner.rs:687-780, :830-905,
 * :938-1135 format them (itoa integers, ryu floats).  Arrays of SagePostColumns may be NULL: the Feature defaults of
 * scoring.rs:576-592 are written (aligned_rt = rt, predicted_* 0.0, delta_*_model 0.999, discriminant 0.0, posterior_error
 * and q-values 1.0).  protein-group columns are always the defaults. */
typedef struct SagePostColumns {
    const float* discriminant_score;
    const float* posterior_error;
    const float* spectrum_q;
    const float* peptide_q;
    const float* protein_q;
    const float* aligned_rt;
    const float* predicted_rt;
    const float* delta_rt_model;
    const float* predicted_ims;
    const float* delta_ims_model;
} SagePostColumns;
enum { SAGE_FORMAT_TSV = 0, SAGE_FORMAT_PIN = 1 };
/* order: [n] row order (indices into features) or NULL; psm_id, spec_ids (spectrum ids, NUL-terminated): [n], indexed like
 * features; filenames: [n_files], indexed by SageFeature.file_id. */
int sage_hip_write_results(const char* path, int format, const SageHostDb* db, const SageFeature* features, uint64_t n,
                           const uint64_t* order, const uint64_t* psm_id, const char* const* filenames, uint32_t n_files,
                           const char* const* spec_ids, const SagePostColumns* post);

/* ---- label-free MS1 quantification (sage-cli runner.rs:562-575: lfq::build_feature_map(..).quantify(..) then
 * fdr::picked_precursor; crates/sage/src/lfq.rs, isotopes.rs, fdr.rs:228-287).  sage_hip_lfq traces MS1 spectra without ion
 * mobility; sage_hip_lfq_im below adds the per-peak mobility column and the mobility window of every feature.
 *   feature map   host: the first confident target feature per peptide; device: the charge x isotope x forward/decoy windows
 *                 (tol_bounds, no FMA), rocPRIM sorts by (rt, peptide, charge, isotope, decoy) and, per 16 384-window page,
 *                 by (mass_lo, rt position)
 *   MS1 peaks     device: mz - PROTON, every peak, stably sorted by mass per spectrum (spectrum.rs:380-412)
 *   traces        device: rt_slice + mass_lookup + Grid::add_entry; every grid cell adds its contributions in the order
 *                 (MS1 spectrum as given, peak, match) — bit-identical to a sequential pass
 *   integration   device, one block per grid: smoothing, spectral angle, time warps (slack 75), scores, peak bounds, areas
 *   q-values      host: picked_precursor, ties of the f32 score kept in grid order
 * Grids are reported in ascending (peptide_idx, charge, decoy) order; charge is 0 when charge states are combined. */
enum { SAGE_LFQ_RETENTION_TIME = 0, SAGE_LFQ_SPECTRAL_ANGLE = 1, SAGE_LFQ_INTENSITY = 2, SAGE_LFQ_HYBRID = 3 };
enum { SAGE_LFQ_APEX = 0, SAGE_LFQ_SUM = 1 };
typedef struct SageLfqSettings {   /* lfq.rs:45-54 */
    int32_t peak_scoring;          /* SAGE_LFQ_RETENTION_TIME .. SAGE_LFQ_HYBRID */
    int32_t integration;           /* SAGE_LFQ_APEX / SAGE_LFQ_SUM */
    double spectral_angle;
    float ppm_tolerance;
    float mobility_pct_tolerance;  /* sage_hip_lfq_im: Tolerance::Pct(-t, t) around Feature.ims; sage_hip_lfq reads no mobility */
    float peptide_q_value;
    uint8_t combine_charge_states;
    uint8_t min_charge, max_charge;/* the search's precursor_charge range */
    uint8_t pad;
} SageLfqSettings;

typedef struct SageLfqInput {
    uint64_t n_features;
    const SageFeature* features;   /* [n]: peptide_idx, label, calcmass, file_id are read (sage_hip_lfq_im: ims, too) */
    const uint32_t* order;         /* [n] confidence order (SageRescoreOutput.order) or NULL: input order */
    const float* aligned_rt;       /* [n], input order */
    const float* peptide_q;        /* [n], input order */
    const SageAlignment* alignments; /* [n_files], indexed by file id (SageRtOutput.alignments) */
    uint32_t n_files;
    uint32_t n_ms1;
    const SageRawBatch* ms1;       /* [n_ms1] raw MS1 spectra (mz, intensities, scan_start_time, file_id), traced in order */
    uint64_t n_peptides;
    const uint16_t* carbon;        /* [n_peptides] mass.rs:78-104 composition of db[i].sequence */
    const uint16_t* sulfur;
    SageLfqSettings settings;
} SageLfqInput;

typedef struct SageLfqOutput {
    /* caller-allocated host arrays of capacity `cap` grids (n_files areas / warps per grid) */
    uint64_t cap;
    uint32_t* peptide_idx;
    uint8_t* charge;               /* 0: charge states combined */
    uint8_t* decoy;
    uint8_t* has_peak;             /* Traces::integrate returned Some */
    uint32_t* peak_rt;             /* best RT bin */
    uint32_t* left;                /* integration bounds [left, right) */
    uint32_t* right;
    double* score;
    double* spectral_angle;
    float* q_value;                /* 1.0 without a peak */
    double* areas;                 /* [cap * n_files] */
    int32_t* warps;                /* [cap * n_files] or NULL */
    double* matrix;                /* [cap * n_files * 3 * 100] or NULL: each grid's summed intensities before smoothing */
    /* filled by the call */
    uint64_t n_grids;              /* grids that received at least one MS1 peak */
    uint64_t n_windows;            /* precursor windows of the feature map */
    uint64_t n_contributions;      /* (peak, window) matches */
    uint64_t passing;              /* target peaks with q <= 0.05 (fdr.rs:270-277) */
    float build_ms, ms1_ms, trace_ms, integrate_ms, device_ms; /* HIP-event times of the stages and of the whole call */
} SageLfqOutput;

/* SAGE_HIP_ERR_INVALID when `cap` is smaller than the grids the call finds (n_grids then holds the number needed). */
int sage_hip_lfq(int device, const SageLfqInput* in, SageLfqOutput* out);

/* sage_hip_lfq for ion-mobility MS1 spectra (lfq.rs:111-127, 267-286, 677-686; spectrum.rs:344-378).  Same inputs and outputs,
 * plus, per MS1 batch, the mobility of every peak:
 *   feature map   every window of a selected feature carries (mobility_lo, mobility_hi) =
 *                 Tolerance::Pct(-mobility_pct_tolerance, mobility_pct_tolerance).bounds(feature.ims) (mass.rs:28-32, f32, no FMA).
 *                 As in the reference, a feature with ims == 0 (no precursor mobility) gets the window [0, 0], and a negative or
 *                 NaN ims gives bounds that no mobility satisfies: the predicate is evaluated as written
 *   MS1 peaks     the stable sort by mass carries the mobility with the intensity
 *   traces        a spectrum WITH mobility keeps a (peak, window) match only if mobility_hi >= m && mobility_lo <= m
 *                 (mass_mobility_lookup; a NaN mobility matches nothing); a spectrum without one is traced as by sage_hip_lfq.
 *                 The order of the contributions, and with it every grid bit, is that of the matches that remain
 * ms1_mobility: [in->n_ms1] or NULL.  NULL, or no spectrum with mobility in any batch: exactly sage_hip_lfq, every output bit. */
typedef struct SageLfqMobility {
    const float* mobility;         /* per peak, indexed like the batch's mz (through its peak_off); NULL: no spectrum has one */
    const uint8_t* has_mobility;   /* [n_spectra] RawSpectrum.mobility is Some; NULL: every spectrum, when `mobility` is given */
} SageLfqMobility;
int sage_hip_lfq_im(int device, const SageLfqInput* in, const SageLfqMobility* ms1_mobility, SageLfqOutput* out);

/* lfq.tsv (sage-cli runner.rs:1182-1235): target grids with a peak, in the order given (rows: indices into the arrays). */
int sage_hip_write_lfq(const char* path, const SageHostDb* db, const SageLfqOutput* grids, const uint64_t* rows, uint64_t n_rows,
                       const char* const* filenames, uint32_t n_files);

/* ---- TMT reporter-ion quantification (sage-cli runner.rs:334-359: tmt::quantify, tmt.rs:193-214, 314-352).  For every
 * spectrum of the batches (the spectra of the quant level, in output order) and every label: the peak
 * select_most_intense_peak(masses, intensities, label, tolerance, Some(-PROTON)) picks (spectrum.rs:134-159).
 *   level 2   SpectrumProcessor::new(take_top_n, deisotope, min_deisotope_mz).process() on the device first — the code of
 *             sage_hip_batch_process_upload with min_peaks 0 — then the extraction over the resident processed peaks
 *   other     mass = mz - PROTON for every peak, extraction over the raw peaks without sorting them (tmt.hip: the selection
 *             is the maximum of a total-order key)
 * intensity[i * n_labels + k]: the picked peak's intensity, 0.0 without one; peak_index (may be NULL): its position in the
 * processed spectrum (level 2) or in the raw spectrum as given (other levels), -1 without one. */
typedef struct SageTmtInput {
    uint32_t n_batches;
    const SageRawBatch* batches;   /* peak_off, mz, intensities (+ precursor_charge at level 2) are read */
    int32_t level;
    uint32_t n_labels;
    const float* labels;           /* reporter m/z, any order, duplicates allowed */
    SageTolerance tolerance;       /* the CLI passes Ppm(-20, 20) */
    uint64_t take_top_n;           /* level 2 only */
    int32_t deisotope;
    float min_deisotope_mz;
} SageTmtInput;

typedef struct SageTmtOutput {
    float* intensity;              /* [n_spectra * n_labels], n_spectra summed over the batches */
    int32_t* peak_index;           /* [n_spectra * n_labels] or NULL */
    /* filled by the call: HIP-event times summed over the batches.  upload_ms: raw peaks to the device (levels != 2);
     * process_ms: upload + process_kernel + compaction (level 2); extract_ms: the extraction kernel; device_ms: the whole
     * call, downloads included */
    float upload_ms, process_ms, extract_ms, device_ms;
} SageTmtOutput;

int sage_hip_tmt(int device, const SageTmtInput* in, SageTmtOutput* out);

/* tmt.tsv (sage-cli runner.rs:1140-1180): filename, scannr (spec_ids as given), ion_injection_time, then one column per header;
 * ryu f32.  file_id indexes filenames. */
int sage_hip_write_tmt(const char* path, const char* const* headers, uint32_t n_labels, uint64_t n_rows, const uint32_t* file_id,
                       const char* const* spec_ids, const float* ion_injection_time, const float* intensity,
                       const char* const* filenames, uint32_t n_files);

/* The competition keys of SageRescoreInput for `n` PSMs given their peptide indices (host work: string keys). */
int sage_hip_hostdb_competition_keys(const SageHostDb* db, const uint32_t* peptide_idx, uint64_t n, uint32_t* peptide_key,
                                 uint32_t* n_peptide_keys, uint32_t* protein_key, uint32_t* n_protein_keys);

/* ---- protein groups and picked protein-group FDR (sage-cli runner.rs:539-549: protein_grouping::generate_protein_groups, then
 * fdr::picked_protein_group; crates/sage/src/protein_grouping.rs:59-386, fdr.rs:192-226).  Additive to ABI 6.
 *   passes        protein_grouping != 0: one pass with threshold clamp(peptide_fdr, 0, 1), one with 1.0; then, and alone when
 *                 protein_grouping == 0, the fallback for every feature still without groups: Peptide::proteins(..) and its length
 *   one pass      device: the peptides of features with label != -1 && peptide_q < threshold (strict; NaN never), compacted in
 *                 ascending order.  host: protein numbering, meta-peptides, groups, edges (sage_hip_group_graph_build).  device:
 *                 the greedy set cover over the edges, then for every peptide of the run still without groups the covered groups
 *                 among its proteins.  host: the strings, once per distinct peptide
 *   competition   features with num_protein_groups == 1, keyed by the group string, side db[peptide].decoy, score
 *                 discriminant_score: the gather per feature and Competition::assign_q_value at 1 % on the device (the code of
 *                 sage_hip_rescore's picked competitions); protein_group_q stays 1.0 elsewhere
 * The cover runs edge-parallel kernels while more live edges remain than SAGE_HIP_COVER_LDS_EDGES (read once per call; default
 * 16384, at most 18432), then one workgroup finishes all remaining rounds with the edges in LDS. */
typedef struct SageGroupInput {
    uint64_t n;
    const SageFeature* features;      /* host, [n]: label and peptide_idx are read */
    const float* peptide_q;           /* [n] */
    const float* discriminant_score;  /* [n] */
    int32_t protein_grouping;         /* input.rs:382 default: 1 */
    float peptide_fdr;                /* protein_grouping_peptide_fdr, input.rs:383 default: 0.01 */
} SageGroupInput;

typedef struct SageGroupStrings SageGroupStrings; /* the distinct protein_groups strings of one call, owned by the library */

typedef struct SageGroupOutput {
    /* caller-allocated host arrays [n], input order */
    uint32_t* num_protein_groups;
    float* protein_group_q;
    uint32_t* string_id;              /* protein_groups of feature i = sage_hip_group_string(strings, string_id[i]) */
    /* filled by the call */
    SageGroupStrings* strings;        /* release with sage_hip_group_strings_free */
    uint64_t n_strings;
    uint64_t passing_protein_group;   /* target groups at 1 % (fdr.rs:105) */
    uint32_t n_groups;                /* of the last pass (threshold 1.0); 0 when protein_grouping == 0 */
    uint32_t n_meta_peptides;         /* of the last pass */
    uint32_t cover_rounds;            /* add_largest_to_cover picks, summed over the passes */
    float device_ms;                  /* HIP-event time of the call's device work, uploads and downloads included */
    double host_graph_ms;             /* wall time of the host graph builder, summed over the passes */
} SageGroupOutput;

int sage_hip_protein_groups(int device, const SageHostDb* db, const SageGroupInput* in, SageGroupOutput* out);
const char* sage_hip_group_string(const SageGroupStrings* strings, uint64_t id); /* NULL when id >= n_strings */
void sage_hip_group_strings_free(SageGroupStrings* strings);

/* The host graph builder alone (no device): ProteinGrouper::build (protein_grouping.rs:171-231) for the ascending, distinct
 * peptide indices `peptides`.  The view's arrays belong to the handle. */
typedef struct SageGroupGraph SageGroupGraph;
typedef struct SageGroupGraphView {
    uint32_t n_proteins, n_meta_peptides, n_groups;
    uint64_t n_edges;
    const uint32_t* protein_id;       /* [n_proteins] ProteinIx -> a protein of the database with that name (sage_hip_hostdb_protein_name) */
    const uint8_t* protein_decoy;     /* [n_proteins] */
    const uint64_t* group_off;        /* [n_groups + 1] into group_proteins */
    const uint32_t* group_proteins;   /* ProteinIx, ascending inside a group */
    const uint64_t* evidence_off;     /* [n_groups + 1] into evidence */
    const uint32_t* evidence;         /* ascending meta-peptide indices of each group */
    const uint32_t* edge_group;       /* [n_edges] */
    const uint32_t* edge_meta;        /* [n_edges] */
} SageGroupGraphView;
int sage_hip_group_graph_build(const SageHostDb* db, const uint32_t* peptides, uint64_t n, SageGroupGraph** out);
int sage_hip_group_graph_view(const SageGroupGraph* graph, SageGroupGraphView* out);
void sage_hip_group_graph_free(SageGroupGraph* graph);
/* name of protein `id` of the database (FASTA accession, without the decoy tag); returns the required buffer size including NUL */
uint64_t sage_hip_hostdb_protein_name(const SageHostDb* db, uint64_t id, char* out, uint64_t cap);

/* sage_hip_write_results with the three protein-group columns of results.sage.tsv (the .pin format has none of them).
 * groups == NULL, or a NULL array in it: that column's default, as sage_hip_write_results writes it. */
typedef struct SageGroupColumns {
    const char* const* strings;          /* [n_strings] NUL-terminated protein_groups strings */
    uint64_t n_strings;
    const uint32_t* string_id;           /* [n] into strings, indexed like features */
    const uint32_t* num_protein_groups;  /* [n] */
    const float* protein_group_q;        /* [n] */
} SageGroupColumns;
int sage_hip_write_results_grouped(const char* path, int format, const SageHostDb* db, const SageFeature* features, uint64_t n,
                                   const uint64_t* order, const uint64_t* psm_id, const char* const* filenames, uint32_t n_files,
                                   const char* const* spec_ids, const SagePostColumns* post, const SageGroupColumns* groups);

/* ---- positional isomers of reported PSMs.  An ADDITION over the reference, which has no counterpart: the scores a
 * localisation step would be built from.  Additive to ABI 6.
 * Two peptides of a host database are positional isomers when their decoy flag, their residue bytes and the multiset of their
 * modification masses are equal — the bit patterns of the non-zero entries of `mods` over the peptide's residues, of nterm and of
 * cterm (each when neither NaN nor 0).  A group has at least two members; groups are numbered by ascending smallest member, members
 * inside a group are ascending peptide indices. */
/* group_of: [n_peptides], 0xFFFFFFFF = the peptide has no isomer.  group_off: [n_groups + 1] into members.
 * Call once with group_off == NULL and members == NULL to get *n_groups and *n_members. */
int sage_hip_hostdb_isomer_groups(const SageHostDb* db, uint32_t* group_of, uint64_t* group_off, uint32_t* members,
                                  uint64_t* n_groups, uint64_t* n_members);

/* Score (scoring.rs:41-67) as score_candidate leaves it (scoring.rs:675-767) */
typedef struct SageCandidateScore {
    double hyperscore;
    float summed_b, summed_y, average_ppm;   /* average_ppm: ppm_difference after the division at the end of score_candidate */
    uint32_t matched_b, matched_y, longest_b, longest_y;
    uint32_t pad;
} SageCandidateScore;

/* For PSM slot s = i * report_psms + r (features / counts as sage_hip_score_resident returned them for this batch and scorer),
 * score the peptides cand_pep[cand_off[s] .. cand_off[s+1]) against spectrum i in the state PSM r was scored in: with chimera,
 * after remove_matched_peaks (scoring.rs:598-644) for PSMs 0 .. r-1 of `features`, exactly as sage_hip_annotate_resident
 * replays it; without chimera, the spectrum as uploaded.  Precursor charge (-> max_fragment_charge): cand_charge[c], or
 * features[s].charge where cand_charge is NULL or cand_charge[c] == 0.  No min_matched_peaks filter: every candidate gets
 * its Score.  out: [cand_off[n * report_psms]].
 * SAGE_HIP_ERR_INVALID, before any launch: cand_off not non-decreasing (or not starting at 0), a non-empty list on a slot with
 * r >= counts[i], a peptide index >= n_peptides, a charge above 254 (the reference's u8 arithmetic around max_fragment_charge has no room left there).  No
 * candidate at all: SAGE_HIP_OK without a launch. */
int sage_hip_score_candidates_resident(SageScorer* scorer, SageDeviceBatch* batch, const SageFeature* features,
                                       const uint32_t* counts, const uint64_t* cand_off, const uint32_t* cand_pep,
                                       const uint8_t* cand_charge, SageCandidateScore* out);
/* HIP-event times of the scorer's last sage_hip_score_candidates_resident call: the whole call on the scorer's stream (uploads
 * and the copy back included) and the kernel alone. */
int sage_hip_last_candidates_timing(const SageScorer* scorer, float* call_ms, float* kernel_ms);

/* ---- site localisation of reported PSMs, Ascore style (after Beausoleil et al. 2006).  An ADDITION over the
 * reference, additive to ABI 6.  Every peak of a spectrum has a depth rank inside its 100-unit mass window (1 = the most
 * intense, ranks above 11 stored as 11); an (ion, fragment charge) item of a candidate matches at depth d (1..10) when its
 * tolerance window — select_most_intense_peak's — holds a peak of rank <= d. */
typedef struct SageDepthCounts {   /* per candidate */
    uint16_t n[10];                /* n[d - 1]: items matched at depth d; non-decreasing */
    uint16_t n_items;              /* N: kinds x ions x fragment charges, as score_candidate walks them */
    uint16_t pad;
} SageDepthCounts;
typedef struct SageLocalisation {  /* per PSM slot */
    double best_score, second_score;  /* peptide scores: sum_d w[d] * S(n[d], N, d) / 7, S = -10 log10 P(Binomial(N, d/100) >= n) */
    double ascore;                 /* S(a[depth], Ns, depth) - S(b[depth], Ns, depth); NaN without a second candidate */
    uint32_t best, second;         /* positions in the slot's list; 0xFFFFFFFF = none */
    uint32_t n_site_items;         /* Ns: items whose ion differs between best and second (f32 bit patterns) */
    uint16_t a[10], b[10];         /* site-determining items of best / of second matched at depth d */
    uint8_t depth;                 /* d*: the depth with the largest a[d] - b[d], ties to the smallest; 0 without a pair */
    uint8_t pad[3];
} SageLocalisation;
/* The lists and their rules are those of sage_hip_score_candidates_resident (same slots, same spectrum states, same
 * SAGE_HIP_ERR_INVALID cases before any launch), and: all candidates of a slot have the residue count and the number of fragment
 * charges of the slot's first candidate, else SAGE_HIP_ERR_INVALID; a candidate of more than 65 535 items: SAGE_HIP_ERR_UNSUPPORTED.
 * per_candidate: [cand_off[n * report_psms]] or NULL.  per_slot: [n * report_psms]; a slot without candidates gets best = second =
 * 0xFFFFFFFF, ascore = NaN and zeros, a slot with one candidate its best and best_score, second = 0xFFFFFFFF, ascore = NaN.
 * No candidate at all: SAGE_HIP_OK without a launch, per_slot untouched. */
int sage_hip_localise_resident(SageScorer* scorer, SageDeviceBatch* batch, const SageFeature* features, const uint32_t* counts,
                               const uint64_t* cand_off, const uint32_t* cand_pep, const uint8_t* cand_charge,
                               SageDepthCounts* per_candidate, SageLocalisation* per_slot);
/* Host only: the f64 arithmetic of DESIGN.md 7f on given counts.  n ([10], may be NULL) with n_items -> depth_scores[10] (S per
 * depth) and *peptide_score, each optional.  a, b ([10]) with n_site_items -> *depth and *ascore (all four or none).  A count
 * above its total: SAGE_HIP_ERR_INVALID. */
int sage_hip_ascore_from_counts(const uint16_t* n, uint32_t n_items, const uint16_t* a, const uint16_t* b, uint32_t n_site_items,
                                double* depth_scores, double* peptide_score, uint8_t* depth, double* ascore);
/* HIP-event times of the scorer's last sage_hip_localise_resident call: the whole call on the scorer's stream (uploads, the copies
 * back and the host's pair selection between the two kernels included) and the two kernels alone. */
int sage_hip_last_localise_timing(const SageScorer* scorer, float* call_ms, float* kernel_ms);

/* ---- protein-level label-free quantification (MaxLFQ: Cox et al. 2014; the roll-up `iq::fast_MaxLFQ` performs on lfq.tsv).  An
 * addition over the reference, additive to ABI 6; the contract is DESIGN.md 7g, stated again in tests/protein_lfq_reference.py.
 * All arithmetic is IEEE f64 without FMA.  For one protein, its rows r in ascending row index, files j, k:
 *   1. L[r][j] = the correctly rounded ln(area) (crlog.h) where area > 0 && area < +inf, else missing.
 *   2. for j < k: d = L[r][j] - L[r][k] over the rows present in both, c_jk their number; the pair is valid when
 *      c_jk >= max(min_ratio_count, 1); m_jk = the median (odd count: the middle element; even: (lo + hi) * 0.5).
 *   3. components of the graph of valid pairs over the files; a component's label is its smallest file index.
 *   4. normal equations of min sum_valid (m_jk - (x_j - x_k))^2: A[j][j] += 1, A[k][k] += 1, A[j][k] -= 1, A[k][j] -= 1,
 *      b[j] = sum_k +-m from +0.0 in ascending k (+m_jk for j < k, -m_kj for k < j); every file that is its component's label is
 *      grounded: row and column zeroed, diagonal 1, b 0.
 *   5. forward elimination without pivoting, pivot row p ascending, rows i > p ascending; a row with A[i][p] == 0.0 is left
 *      untouched, else f = A[i][p] / A[p][p], A[i][c] -= f * A[p][c] for c = p .. n_files - 1 ascending, b[i] -= f * b[p].  Back
 *      substitution, i descending: s = b[i]; s -= A[i][c] * x[c] for c ascending from i + 1; x[i] = s / A[i][i].  A zero or
 *      non-finite pivot: SAGE_HIP_ERR_INTERNAL.
 *   6. col[j] = sum_r L[r][j] from +0.0 in ascending r, cnt[j] the number of present rows; per component over its members in
 *      ascending j: T = sum col, N = sum cnt, S = sum x; N == 0: every member NaN; else x[j] + (T / N - S / |component|).
 * log_abundance: natural log, NaN = not quantified; component: the label, 0xFFFFFFFF where not quantified; n_rows_used: the rows
 * whose protein_of_row names the protein; n_components: among quantified files; intensity = det_exp(log_abundance) (detmath.h),
 * 0.0 where not quantified.  pair_median / pair_count (each may be NULL): [n_proteins * n_files (n_files - 1) / 2], (j, k) in
 * lexicographic order; the median is NaN where the pair is not valid.
 * protein_of_row: ids 0 .. n_proteins - 1 in any row order, 0xFFFFFFFF = the row is ignored; another id >= n_proteins or a NULL
 * array: SAGE_HIP_ERR_INVALID.  More than 65 535 files: SAGE_HIP_ERR_UNSUPPORTED.  n_proteins == 0: SAGE_HIP_OK, nothing
 * written; n_rows == 0 or n_files == 0: SAGE_HIP_OK without a launch, every protein not quantified.
 * Proteins go through the device in batches whose tables stay below SAGE_HIP_PLFQ_WORKSPACE_MB; n_batches counts
 * them.  log_ms: upload, grouping and logarithms; median_ms / solve_ms: the two kernels summed over the batches; device_ms: all
 * of it, copies back included (HIP events). */
typedef struct SageProteinLfqInput {
    uint64_t n_rows;
    uint32_t n_files, n_proteins, min_ratio_count;
    const double* areas;              /* [n_rows * n_files] */
    const uint32_t* protein_of_row;   /* [n_rows] */
} SageProteinLfqInput;

typedef struct SageProteinLfqOutput {
    double* log_abundance;            /* [n_proteins * n_files] */
    double* intensity;
    uint32_t* component;
    uint32_t* n_rows_used;            /* [n_proteins] */
    uint32_t* n_components;
    double* pair_median;              /* optional */
    uint32_t* pair_count;
    float log_ms, median_ms, solve_ms, device_ms;
    uint32_t n_batches;
} SageProteinLfqOutput;

int sage_hip_protein_lfq(int device, const SageProteinLfqInput* in, SageProteinLfqOutput* out);

/* protein_lfq.tsv: proteins, n_precursors, n_components, then one intensity per file (ryu f64; 0.0 where not quantified), one row
 * per entry of `rows` (protein ids of `result`, in the order given); protein_names[id] is written as the `proteins` field. */
int sage_hip_write_protein_lfq(const char* path, const char* const* protein_names, uint32_t n_proteins, const uint32_t* rows,
                               uint32_t n_out, const SageProteinLfqOutput* result, const char* const* filenames, uint32_t n_files);

/* ---- precursor purity of reported PSMs from MS1 scans ("precursor ion fraction", "isolation interference").  An addition over the
 * reference, additive to ABI 6; the contract is DESIGN.md 7h and sage_amd/csrc/purity.h, stated again in tests/purity_reference.py.
 * One query: an MS1 spectrum (raw m/z, peaks in the order given), a precursor m/z, a charge z (0: unknown), isolation offsets
 * (lo, hi) in Da (either NaN, or either array NULL: the settings' default pair).  All m/z arithmetic is f32 without FMA.
 *   window    [mz + lo, mz + hi], both ends inside; a NaN m/z is in no interval.
 *   envelope  c_k = mz + (k * NEUTRON) / z, k = 0 .. max_isotope (z == 0: c_0 = mz alone); a peak of the window is matched when it
 *             lies inside the ppm bounds (Tolerance::bounds of Ppm(-t, t)) of at least one c_k, and is counted once.
 *   below     every peak of the spectrum, in the window or not, inside the ppm bounds of mz - NEUTRON / z (z == 0: none).
 *   total, matched, below: f64 sums of (double)intensity from +0.0, peak after peak in ascending position in the spectrum; NaN, +-inf,
 *   negative and -0.0 intensities pass through.  purity = (float)(matched / total), stored as computed; -1.0f (with zero sums and
 *   counts) when no peak is in the window or ms1_index is UINT64_MAX.
 * Checked before the device is touched, each SAGE_HIP_ERR_INVALID: a NULL array with n_queries > 0, an ms1_index that is neither
 * UINT64_MAX nor below the number of spectra, max_isotope > 16, a ppm_tolerance that is negative or not finite, a peak_off that
 * decreases.  A spectrum of more than 2^31 - 1 peaks: SAGE_HIP_ERR_UNSUPPORTED.  No query, or none with a spectrum: SAGE_HIP_OK
 * without a launch.  The MS1 batches go through the device one at a time (a batch without a query is skipped), so device memory is
 * bounded by the largest batch.  A spectrum whose m/z are non-decreasing and NaN-free is read by partition points (n_sorted_spectra),
 * any other is scanned whole (n_scanned_spectra); SAGE_HIP_PURITY_SCAN=1 scans all; the results are the same bits. */
typedef struct SagePuritySettings {
    float ppm_tolerance, default_isolation_lo, default_isolation_hi;
    uint32_t max_isotope;
} SagePuritySettings;

typedef struct SagePurityInput {
    uint32_t n_ms1;
    const SageRawBatch* ms1;          /* peak_off, mz, intensities are read */
    uint64_t n_queries;
    const uint64_t* ms1_index;        /* spectrum number counted through the batches in order; UINT64_MAX: none */
    const float* precursor_mz;
    const uint8_t* charge;
    const float* isolation_lo;        /* either NULL: the default pair for every query */
    const float* isolation_hi;
    SagePuritySettings settings;
} SagePurityInput;

typedef struct SagePurityOutput {     /* caller-allocated, [n_queries] each */
    uint32_t* n_window;
    uint32_t* n_matched;
    double* total;
    double* matched;
    double* below;
    float* purity;
    uint64_t n_sorted_spectra, n_scanned_spectra; /* spectra with at least one query, by route */
    float upload_ms, kernel_ms, device_ms;        /* HIP events, summed over the batches */
} SagePurityOutput;

int sage_hip_precursor_purity(int device, const SagePurityInput* in, SagePurityOutput* out);

/* purity.sage.tsv: psm_id, filename, scannr, charge, ms1_scannr (empty where ms1_ids[r] is NULL or ""), isolation_lo, isolation_hi,
 * peaks_in_window, peaks_matched, total_intensity, precursor_intensity, below_intensity, purity; one row per entry, in the order
 * given; f32 / f64 as ryu writes them.  `result` holds [n_rows] arrays. */
int sage_hip_write_purity(const char* path, uint64_t n_rows, const uint64_t* psm_id, const uint32_t* file_id, const char* const* spec_ids,
                          const uint8_t* charge, const char* const* ms1_ids, const float* isolation_lo, const float* isolation_hi,
                          const SagePurityOutput* result, const char* const* filenames, uint32_t n_files);

/* ---- protein-level roll-up of TMT reporter intensities (what follows tmt.tsv in every TMT workflow: filter, equalise the channel
 * loading, one abundance per protein and channel).  An addition over the reference, additive to ABI 6; the contract is DESIGN.md 7i
 * and sage_amd/csrc/tmt_rollup.h, stated again in tests/tmt_rollup_reference.py.  One call is one plex: rows that share their
 * channels.  All arithmetic is IEEE f64 without FMA.  For rows r, channels k, groups g:
 *   1. v = (double)intensity[r][k]; the cell is present when v > 0 && v < +inf (NaN, +-0.0, negatives and +inf are missing).  A row
 *      is used when group_of_row[r] != 0xFFFFFFFF and it has at least max(min_present, 1) present cells.
 *   2. block b holds the input rows [1024 b, 1024 (b + 1)).  P[b][k] = the sum of the present cells of channel k over the used rows
 *      of block b, from +0.0 in ascending row index; S[k] (column_sum) = the sum of P[b][k] from +0.0 in ascending b; C[k] = the
 *      number of present cells of channel k over the used rows.
 *   3. normalise None: f[k] = 1.0.  Total: M = (the sum of S[k] over the channels with C[k] > 0, ascending k, from +0.0) / their
 *      number; f[k] (factor) = M / S[k] where C[k] > 0, else 1.0.  w[r][k] = v * f[k].
 *   4. summary Sum: abundance[g][k] = the sum of w[r][k] over the used rows of g whose cell is present, from +0.0 in ascending row
 *      index; n_cells[g][k] their number; log_abundance = the correctly rounded ln(abundance) (crlog.h) where n_cells > 0, else NaN
 *      with abundance +0.0.
 *   5. summary Median: l = ln(w) (correctly rounded) of every present cell; the row's centre c[r] = (the sum of its present l,
 *      ascending k, from +0.0) / their number; d[r][k] = l - c[r]; med[g][k] = the exact median of d over the used rows of g whose
 *      cell is present (ranks (n - 1) / 2 and n / 2 in ascending order; odd n: the middle element, even: (lo + hi) * 0.5);
 *      a[g] = (the sum of c[r] over the used rows of g, ascending row index, from +0.0) / n_rows_used[g];
 *      log_abundance = med + a, NaN where n_cells == 0; abundance = det_exp(log_abundance) (detmath.h), 0.0 where not quantified.
 * Checked before the device is touched: a NULL array with n_rows > 0, a group id >= n_groups other than 0xFFFFFFFF, normalise or
 * summary out of range, n_labels == 0 with n_rows > 0: SAGE_HIP_ERR_INVALID.  n_labels > 65 535 or n_rows >= 2^31:
 * SAGE_HIP_ERR_UNSUPPORTED.  n_groups == 0: SAGE_HIP_OK, nothing written.  n_rows == 0, or no used row: SAGE_HIP_OK without a
 * summary launch, every group not quantified, factors 1.0, column sums 0.0.
 * n_used_rows: the used rows.  n_long_groups: the groups whose medians were selected by passes over their columns in global memory
 * (more used rows than a wavefront's LDS slice holds, 1 024; 0 for Sum).  n_label_slabs: the slabs of 64 channels a wavefront of
 * the summary kernel walks for one group, ceil(n_labels / 64); 0 without a summary launch.  norm_ms: upload, presence, grouping,
 * column sums and factors; summary_ms: centres and the summary kernels; device_ms: all of it, copies back included (HIP events). */
enum { SAGE_TMT_NORMALISE_NONE = 0, SAGE_TMT_NORMALISE_TOTAL = 1 };
enum { SAGE_TMT_SUMMARY_SUM = 0, SAGE_TMT_SUMMARY_MEDIAN = 1 };

typedef struct SageTmtRollupInput {
    uint64_t n_rows;
    uint32_t n_labels, n_groups, min_present;
    int32_t normalise, summary;
    const float* intensity;           /* [n_rows * n_labels], row-major (SageTmtOutput.intensity) */
    const uint32_t* group_of_row;     /* [n_rows] */
} SageTmtRollupInput;

typedef struct SageTmtRollupOutput {  /* caller-allocated */
    double* abundance;                /* [n_groups * n_labels] */
    double* log_abundance;
    uint32_t* n_cells;
    uint32_t* n_rows_used;            /* [n_groups] */
    double* factor;                   /* [n_labels] */
    double* column_sum;
    uint64_t n_used_rows;
    uint32_t n_long_groups, n_label_slabs;
    float norm_ms, summary_ms, device_ms;
} SageTmtRollupOutput;

int sage_hip_tmt_rollup(int device, const SageTmtRollupInput* in, SageTmtRollupOutput* out);

/* tmt_proteins.tsv / tmt_peptides.tsv: `first_header` ("proteins" or "peptide"), plex, n_psms, n_peptides, then one abundance per
 * channel header (ryu f64; 0.0 where not quantified); one row per entry, in the order given: names[r], plex[r], n_psms[r],
 * n_peptides[r], abundance[r * n_labels ..]. */
int sage_hip_write_tmt_rollup(const char* path, const char* first_header, const char* const* headers, uint32_t n_labels, uint64_t n_out,
                              const char* const* names, const uint32_t* plex, const uint32_t* n_psms, const uint32_t* n_peptides,
                              const double* abundance);

const char* sage_hip_last_error(void);
int sage_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SAGE_HIP_H */
