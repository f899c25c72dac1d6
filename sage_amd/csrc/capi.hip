// capi.hip — the scorer of the C ABI declared in include/sage_hip.h: scorer handles, batch upload, and the whole scoring engine —
// everything a resident or streaming scoring step calls per step is in this one translation unit.  The other entry points:
// capi_db.hip (the device database), capi_psm.hip (the steps over reported PSMs), capi_host.cpp (what takes no scorer); the
// handle structs: capi_state.h.
#include <algorithm>
#include <chrono>
#include <future>

#include "capi_state.h"
#include "crlog.h"

extern "C" {

// DevScorer::tol_mode (core.h: TolMode).  TOL_SYM: a symmetric ppm fragment tolerance — one division per Tolerance::bounds
// (mass.rs:21-35).  TOL_FAST: the rescoring instance with the short divisions by 1e6 and by 3 (core.h: div_const_fast —
// the correctly rounded quotient for every dividend of FAST_DIV_LO <= |x| <= FAST_DIV_HI) may score for this scorer: the
// dividends are bounded from the database's ion table — an ion for the charge-3 m/z (scoring.rs:707), |ion| / charge (a u8:
// <= 255) times each bound of a ppm tolerance — and whatever does not fit keeps the IEEE sequence: a table with a zero, an
// infinite or a NaN entry, a ppm bound of zero, absurd magnitudes.
static uint32_t scorer_tol_mode(const sagecore::Tol& t, uint32_t ion_lo_bits, uint32_t ion_hi_bits) {
    uint32_t mode = 0;
    if (t.kind == 0 && t.lo == -t.hi) mode |= sagecore::TOL_SYM;
    if (ion_lo_bits > ion_hi_bits) return mode;  // (no ions at all)
    float ion_lo, ion_hi;
    std::memcpy(&ion_lo, &ion_lo_bits, 4);
    std::memcpy(&ion_hi, &ion_hi_bits, 4);
    const double lo = sagecore::FAST_DIV_LO, hi = sagecore::FAST_DIV_HI;
    bool ok = ion_lo >= lo && ion_hi <= hi;  // (NaN: its bits sort above +inf, the comparison fails)
    if (ok && t.kind == 0)
        for (const float b : {t.lo, t.hi}) {
            const double a = std::fabs((double)b);
            // (a factor of two either side for the rounding of the f32 quotient |ion| / charge and of the f32 product)
            ok = ok && a > 0.0 && (double)ion_lo / 255.0 * a >= 2.0 * lo && (double)ion_hi * a <= 0.5 * hi;
        }
    if (ok) mode |= sagecore::TOL_FAST;
    return mode;
}

static int scorer_init(SageScorer* sp, SageDeviceDb* db, const SageScorerParams* p) {
    SageScorer* s = sp;
    s->db = db;
    s->params = *p;
    DevScorer& d = s->dev;
    d.precursor_tol = {p->precursor_tol.kind, p->precursor_tol.lo, p->precursor_tol.hi};
    d.fragment_tol = {p->fragment_tol.kind, p->fragment_tol.lo, p->fragment_tol.hi};
    d.pbm_reach = sagecore::pbm_reach_of(d.fragment_tol);
    d.min_matched_peaks = p->min_matched_peaks;
    d.min_isotope_err = p->min_isotope_err;
    d.max_isotope_err = p->max_isotope_err;
    d.min_precursor_charge = p->min_precursor_charge;
    d.max_precursor_charge = p->max_precursor_charge;
    d.override_precursor_charge = p->override_precursor_charge;
    d.max_fragment_charge = p->max_fragment_charge;
    d.chimera = p->chimera;
    d.report_psms = p->report_psms;
    d.wide_window = p->wide_window;
    d.score_type = p->score_type;
    d.kmax = std::max<uint32_t>(50, 2 * p->report_psms);
    const uint32_t n_iso = (uint32_t)(p->max_isotope_err - p->min_isotope_err) + 1;
    const uint32_t n_z = (uint32_t)(p->max_precursor_charge - p->min_precursor_charge) + 1;
    d.list_cap = d.kmax * (std::max(n_iso, n_z) + 1);
    d.wcap = 1024;
    d.dbg_flags = 0;
    if (const char* e = getenv("SAGE_HIP_DEBUG_FLAGS")) d.dbg_flags = (uint32_t)atoi(e);
    s->hand_rows = (d.dbg_flags & 131072u) == 0u;  // (131072: tests and A/B runs keep the hand-over arrays indexed by spectrum)
    d.prune_min = (d.dbg_flags & 4096u) ? 0u : d.min_matched_peaks;  // (4096: tests and A/B runs switch the rescoring prune off)
    d.rescore_general = 0;
    if (const char* e = getenv("SAGE_HIP_RESCORE_GENERAL")) d.rescore_general = atoi(e) != 0 ? RESCORE_GENERAL_CHIMERA : 0u;
    {
        // the instance compiled for two ion kinds, the first n-terminal (a / b / c), the second not — {b, y}, the reference's default:
        // decided here, once per scorer, from the database's kinds (SAGE_HIP_RESCORE_KINDS_GENERAL=1: tests and A/B runs keep the general one)
        const DevDbView& v = db->view;
        bool kinds2 = v.n_kinds == 2u && v.ion_kinds[0] <= 2 && v.ion_kinds[1] > 2;
        if (const char* e = getenv("SAGE_HIP_RESCORE_KINDS_GENERAL")) kinds2 = kinds2 && atoi(e) == 0;
        if (!kinds2) d.rescore_general |= RESCORE_GENERAL_KINDS;
    }
    d.exact = 0;
    d.xcd_chunk = 1024;
    if (const char* e = getenv("SAGE_HIP_XCD_CHUNK")) d.xcd_chunk = (uint32_t)std::max(0, atoi(e));
    // (bit 31: heaviest precursors first — the default since round 6: the expensive spectra start first and the step's tail is made
    // of cheap ones; a rank's 62 500-spectrum C3 shard -7 %, C2 -4 %, 500 000 spectra -1 %: scripts/experiments/r06_lab/gpu_r7y.sh)
    // Batches that may hold large windows keep the ascending order unless the variable asks (C4 +1 % with it, C5 -0.5 %: their
    // steps are the count kernel's, which takes the spectra in queue order): plan_step.
    {
        const char* e = getenv("SAGE_HIP_SCHED_DESC");
        if (!e || atoi(e)) d.xcd_chunk |= 0x80000000u;
        s->sched_desc_forced = e != nullptr;
    }
    if (const char* e = getenv("SAGE_HIP_EXACT")) s->exact_always = atoi(e) != 0;
    if (const char* e = getenv("SAGE_HIP_FUSED")) s->fused = atoi(e) != 0;
    if (const char* e = getenv("SAGE_HIP_ONE_LANE")) s->two_lanes = atoi(e) == 0;
    if (const char* e = getenv("SAGE_HIP_SEARCH_LAG")) s->search_lag = (uint32_t)std::max(0, atoi(e));
    if (const char* e = getenv("SAGE_HIP_REPLAY_WAVE_MAX")) s->replay_split = (uint64_t)atoll(e) & 0xFFFFFFFFull;
    if (const char* e = getenv("SAGE_HIP_REPLAY_LANE_MAX")) s->replay_split |= (uint64_t)(uint32_t)atoll(e) << 32;
    if (const char* e = getenv("SAGE_HIP_ONE_LAUNCH")) s->one_launch = atoi(e) != 0;
#ifndef SAGE_HIP_EXPERIMENTS
    // the losing first-pass experiments of DESIGN.md 4.7 (search_kernel, the fused kernel as the first pass) are compiled into
    // builds with -DSAGE_HIP_EXPERIMENTS only (scripts/variants.sh exp:"-DSAGE_HIP_EXPERIMENTS")
    if (s->one_launch || s->fused || getenv("SAGE_HIP_SEARCH_LAG"))
        return fail(SAGE_HIP_ERR_UNSUPPORTED, "SAGE_HIP_ONE_LAUNCH / SAGE_HIP_FUSED / SAGE_HIP_SEARCH_LAG need a build with -DSAGE_HIP_EXPERIMENTS");
#endif
    if (const char* e = getenv("SAGE_HIP_NO_ZEROCOPY")) s->zero_copy = atoi(e) == 0;
    if (const char* e = getenv("SAGE_HIP_NO_FAST_TIES")) s->fast_ties = atoi(e) == 0;
    if (const char* e = getenv("SAGE_HIP_WCAP")) d.wcap = (uint32_t)std::min(16384, std::max(64, atoi(e)));  // (32-bit heap keys need <= 65536)
    if (const char* e = getenv("SAGE_HIP_CHUNK")) s->chunk = (uint32_t)std::min(1 << 22, std::max(64, atoi(e)));
    HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&s->up_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&s->down_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&s->side_stream, hipStreamNonBlocking));
    if (const char* e = getenv("SAGE_HIP_WAYS")) s->ways = (uint32_t)std::min(4, std::max(1, atoi(e)));
    // cheap ties: only where the tied candidates' records are final whichever wins (one reported PSM, no chimera rounds)
    if (p->report_psms != 1 || p->chimera) s->fast_ties = false;
    // ... and only where a spectrum's window counts fit the LDS rescore_kernel replays them in (the peak bitmap + the peak table,
    // dead by then: kernels.hip FAST_TIE_WORDS; wcap <= 2560 — the default is 1024, SAGE_HIP_WCAP raises it).  Larger windows
    // settle their ties through the exact retry pass.
    if ((d.wcap + 1) / 2 > fast_tie_lds_words()) s->fast_ties = false;
    s->cnt_stride = 4u + (((d.wcap + 1) / 2 + 3u) & ~3u);  // (kernels.hip: CNT_ROW_HEADER)
    // Peptides of more than 1023 residues (the reference has no limit: database.rs:96-115 `max_len` is the user's): their ion
    // indices do not fit the one-register Run state of the production rescoring kernel, so such a database takes the same slow,
    // general instances as lists wider than a wavefront, with rescore_big_kernel's two-register Run form.
    d.long_runs = db->max_len > 1023 ? 1u : 0u;
    d.big_path = (d.kmax > 64 || d.long_runs) ? 1u : 0u;
    d.tol_mode = scorer_tol_mode(d.fragment_tol, db->ion_lo_bits, db->ion_hi_bits);
    // (the instance with the short divisions is opt-in: 97 vector instructions and 13 division sequences shorter on paper, identical
    // results — and 1-2 % SLOWER on C3, 2.755 against 2.70-2.73 ms per 500 000 spectra: profiles/r05_C3_short_divisions.txt)
    if (!getenv("SAGE_HIP_SHORT_DIVISIONS")) d.tol_mode &= ~(uint32_t)sagecore::TOL_FAST;
    if (d.big_path) {
        // report_psms > 32: preliminary lists of up to 256 candidates, wider than a wavefront.  The BIGK kernels (kernels.hip): heaps
        // in LDS, every trim exact (no order-free trims, hence no retry pass), rescoring 64 candidates at a time.
        s->kstride = ((d.kmax + 63) / 64) * 64;
        HIP_TRY((hipError_t)bigk_kernel_prepare(160 * 1024));
        s->exact_always = true;
        s->fused = s->one_launch = false;
        s->ways = 1;
    }
    for (hipStream_t& ws : s->way_stream) HIP_TRY(hipStreamCreateWithFlags(&ws, hipStreamNonBlocking));
    HIP_TRY(s->way_begin.create(true));
    for (Event& e : s->way_end) HIP_TRY(e.create(true));
    HIP_TRY(s->side_fork.create(false));
    HIP_TRY(s->side_join.create(false));
    for (OutSet& o : s->outs) {
        for (auto& e : o.ev) HIP_TRY(e.create(true));
        HIP_TRY(o.comp_done.create(false));
        HIP_TRY(o.down_done.create(false));
        HIP_TRY(o.counters.alloc(2 * CTR_COUNT));
        HIP_TRY(hipHostMalloc((void**)&o.h_counters, 2 * CTR_COUNT * 4, hipHostMallocDefault));
        HIP_TRY(hipHostGetDevicePointer((void**)&o.h_counters_view, o.h_counters, 0));
    }
    for (SageDeviceBatch& b : s->slots) {
        b.device = db->device;
        HIP_TRY(b.up_done.create(false));
    }
    // lnfact (scoring.rs:170-177) tabulated on the host with the SAME correctly rounded ln the kernels use (crlog.h): the
    // factorial terms do not depend on the host's libm
    std::vector<double> tbl(131072);  // every u16 count and every sum of two (Score.matched_b/y are u16, scoring.rs:17-30)
    tbl[0] = 1.0;
    for (uint32_t n = 1; n < tbl.size(); n++) {
        const double x = (double)n;
        tbl[n] = x * sagecore::cr_log(x) - x + 0.5 * sagecore::cr_log(x) + 0.5 * sagecore::cr_log(M_PI * 2.0 * x);
    }
    HIP_TRY(s->lnfact.upload(tbl.data(), tbl.size()));
    // large-window kernel: persistent workgroups, as many as the LDS tiles allow to be resident
    {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, db->device));
        const size_t tile_lds = ((size_t)1 << db->view.tile_shift) * 2 + 12 * 1024;  // counters + bitmap + windows (typical)
        const uint32_t per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / tile_lds));
        s->tile_blocks = (uint32_t)prop.multiProcessorCount * per_cu;
        const size_t tile_lds8 = ((size_t)1 << db->view.tile_shift) + 14 * 1024;
        s->tile_blocks8 = (uint32_t)prop.multiProcessorCount * (uint32_t)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / tile_lds8));
        if (const char* e = getenv("SAGE_HIP_TILE_BLOCKS")) s->tile_blocks = s->tile_blocks8 = (uint32_t)std::max(1, atoi(e));
        if (const char* e = getenv("SAGE_HIP_NO_U8")) s->cnt8 = atoi(e) == 0;
        if (const char* e = getenv("SAGE_HIP_NO_REUSE")) s->reuse_counts = atoi(e) == 0;
        HIP_TRY((hipError_t)tile_kernel_prepare(160 * 1024));
        HIP_TRY((hipError_t)spectrum_kernel_prepare(160 * 1024));
    }
    s->qmax = queries_per_spectrum(d);
    if (const char* e = getenv("SAGE_HIP_PHASE_CLOCKS")) {
        if (atoi(e) > 0) {
            HIP_TRY(s->dbg.alloc(DBG_TOTAL_WORDS));  // (the phase block + the prune counters behind it: device_types.h)
            HIP_TRY(hipMemset(s->dbg.p, 0, DBG_TOTAL_WORDS * 8));
        }
    }
    return SAGE_HIP_OK;
}

static void scorer_release(SageScorer* s) {
    (void)hipSetDevice(s->db->device);
    for (hipStream_t st : {s->stream, s->up_stream, s->down_stream, s->side_stream, s->way_stream[0], s->way_stream[1], s->way_stream[2]})
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    delete s;
}

int sage_hip_scorer_create(SageDeviceDb* db, const SageScorerParams* p, SageScorer** out) {
    if (!db || !p || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    if (p->report_psms == 0) return fail(SAGE_HIP_ERR_INVALID, "report_psms must be >= 1");
    // (trim_hits keeps max(50, 2 * report_psms) candidates, scoring.rs:322-329, and the reference has no cap; lists that no longer fit
    // a compute unit's LDS live in a global-memory workspace — plan_step: hugebuf.  16-bit fields of the large-window
    // records bound the list at 65 534 entries.)
    if (p->report_psms > 32767) return fail(SAGE_HIP_ERR_UNSUPPORTED, "report_psms > 32767");
    if (p->min_isotope_err > p->max_isotope_err) return fail(SAGE_HIP_ERR_INVALID, "min_isotope_err > max_isotope_err");
    if (p->min_precursor_charge > p->max_precursor_charge || p->min_precursor_charge == 0)
        return fail(SAGE_HIP_ERR_INVALID, "precursor charge range must be [lo >= 1, hi >= lo]");
    if (p->score_type != 0 && p->score_type != 1) return fail(SAGE_HIP_ERR_INVALID, "unknown score_type");
    HIP_TRY(hipSetDevice(db->device));
    SageScorer* s = new SageScorer();
    const int rc = scorer_init(s, db, p);
    if (rc != SAGE_HIP_OK) {
        s->db = db;
        scorer_release(s);
        return rc;
    }
    *out = s;
    return SAGE_HIP_OK;
}

// Scorer::score takes &self and is called from every rayon worker at once (scoring.rs:300, runner.rs:311-325).  One handle
// may be shared between host threads — its calls then run one after the other — and a clone is a second handle on the same
// device database with its own streams and working set, for callers that want their batches scored concurrently.
int sage_hip_scorer_clone(SageScorer* scorer, SageScorer** out) {
    if (!scorer || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    return sage_hip_scorer_create(scorer->db, &scorer->params, out);
}

void sage_hip_scorer_destroy(SageScorer* s) {
    if (!s) return;
    scorer_release(s);
}

// ---- batches ---------------------------------------------------------------------------------------------------------------
// the device-side address of page-locked, mapped host memory (sage_hip_host_alloc / hipHostMalloc); null for anything else
static void* device_view(const void* p) {
    if (!p) return nullptr;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return at.type == hipMemoryTypeHost ? at.devicePointer : nullptr;
}
// ... without asking the driver, for memory this library page-locked itself (sage_hip_host_alloc keeps a registry of its blocks: a
// caller that scores batch after batch into the same result arrays — every step of a resident loop — otherwise pays two driver
// queries, ~5 us each, in front of the step's first launch).  Only those blocks: for page-locked memory of any other origin the
// library cannot know when it is unpinned or freed, so it asks every time.
struct HostBlock {
    const unsigned char* host;
    unsigned char* dev;
    size_t bytes;
};
static std::mutex g_blocks_mu;
static std::vector<HostBlock> g_blocks;
static void* device_view_cached(const void* p) {
    if (!p) return nullptr;
    {
        std::lock_guard<std::mutex> lock(g_blocks_mu);
        for (const HostBlock& b : g_blocks)
            if ((const unsigned char*)p >= b.host && (const unsigned char*)p < b.host + b.bytes) return b.dev + ((const unsigned char*)p - b.host);
    }
    return device_view(p);
}
static bool is_page_locked(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // plain pageable memory: "invalid value", not an error for us
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// What a batch looks like to the narrow kernel, from (a sample of) its spectra: the mean candidate-window size picks the
// matching variant, the largest one says whether the large-window kernels have to be launched at all.
// The per-spectrum isolation-window kinds of the entry point in progress (sage_hip_*_kinds), for the upload paths and the window
// estimate below it; set and cleared under the scorer's mutex.
struct KindScope {
    SageScorer* s;
    KindScope(SageScorer* s_, const uint8_t* kinds) : s(s_) { s->iso_kind = kinds; }
    ~KindScope() { s->iso_kind = nullptr; }
};
struct WindowEstimate {
    uint32_t probe;       // narrow kernel variant (DevBatchView::probe)
    bool maybe_wide;      // some window may exceed DevScorer::wcap (a sample cannot rule it out: callers re-run on a wrong "no")
};
static WindowEstimate choose_probe(const SageScorer* s, uint32_t n, const float* precursor_mz, const uint8_t* precursor_charge,
                                   const float* isolation_lo, const float* isolation_hi, const uint8_t* iso_kind) {
    const SageScorerParams& p = s->params;
    const std::vector<float>& pm = s->db->h_pep_mono;
    const uint32_t step = std::max<uint32_t>(1, n / 1024);  // (each sample costs two searches over the whole peptide list: ~0.2 us)
    double sum = 0.0;
    uint64_t widest = 0;
    uint32_t cnt = 0;
    for (uint32_t i = 0; i < n; i += step, cnt++) {
        const bool ranged = p.wide_window || precursor_charge[i] == 0 || p.override_precursor_charge;  // scoring.rs:423, 437, 442
        const uint32_t z0 = ranged ? p.min_precursor_charge : precursor_charge[i], z1 = ranged ? p.max_precursor_charge : precursor_charge[i];
        for (uint32_t z = z0; z <= z1; z++) {
            const float center = (precursor_mz[i] - sagecore::PROTON) * (float)z;
            sagecore::Tol tol{p.precursor_tol.kind, p.precursor_tol.lo, p.precursor_tol.hi};
            if (p.wide_window) {
                float lo = -2.4f, hi = 2.4f;
                int kind = 2;
                if (isolation_lo && isolation_hi && isolation_lo[i] == isolation_lo[i] && isolation_hi[i] == isolation_hi[i]) {
                    lo = isolation_lo[i];
                    hi = isolation_hi[i];
                    kind = iso_kind ? iso_kind[i] : 2;
                }
                tol = sagecore::Tol{kind, lo * (float)z, hi * (float)z};
            }
            float lo, hi;
            sagecore::tol_bounds(tol, center, lo, hi);
            // the window's upper end is searched for from its lower end, in doubling strides (windows are short next to the list)
            const auto first = std::lower_bound(pm.begin(), pm.end(), lo);
            size_t reach = 64;
            while ((size_t)(pm.end() - first) > reach && first[reach] <= hi) reach *= 2;
            const auto last = std::upper_bound(first, (size_t)(pm.end() - first) > reach ? first + reach : pm.end(), hi);
            const uint64_t wdw = (uint64_t)(last - first);
            if (z == z0) sum += (double)wdw;
            widest = std::max(widest, wdw);
        }
    }
    const double mean_window = cnt ? sum / cnt : 0.0;
    WindowEstimate e;
    // The matching variant: table lookups per (peak, fragment charge) window ("probe") unless the windows hold next to nothing.
    // Round 5 re-measured the threshold (round 2 had put it at 96 candidates, before the small tiles, the position table of the
    // peptide masses and the DPP scans made the probe variant 2-3x faster): C2, mean window ~25 candidates — preliminary kernel 0.82 ms
    // streaming against 0.33 ms probing per 50 000 spectra (the step 0.70 -> 0.50 ms); the heaviest 1/32 of C3 (mean window 67
    // candidates of ~80 fragments each) 0.79 against 0.12 ms per 15 600 spectra (profiles/r05_shard_sizes.txt).  Streaming walks
    // candidates x fragments entries with a binary search over the windows each; it can only win where that product is tiny.
    e.probe = mean_window > 4.0 ? 1u : 0u;
    if (const char* v = getenv("SAGE_HIP_NARROW")) e.probe = std::string(v) == "probe" ? 1u : std::string(v) == "stream" ? 0u : e.probe;
    // (a quarter of headroom between the widest sampled window and the capacity: isotope errors shift the centre, the sample is thin)
    e.maybe_wide = widest + widest / 4 + 2 > s->dev.wcap;
    if (const char* v = getenv("SAGE_HIP_ASSUME_NARROW")) e.maybe_wide = atoi(v) == 0;  // (tests: force the wrong guess and its repair)
    return e;
}

// largest fragment charge any spectrum of a batch can ask for (scoring.rs:239-247)
static uint32_t batch_fzcap(const SageScorerParams& p, uint32_t zmax, bool any_unknown) {
    uint32_t fzcap = 1;
    const bool ranged = p.wide_window || p.override_precursor_charge || any_unknown;
    for (uint32_t z = 1; z <= 255; z++) {
        const bool used = (ranged && z >= p.min_precursor_charge && z <= p.max_precursor_charge) ||
                          (!p.wide_window && !p.override_precursor_charge && z <= zmax);
        if (used) fzcap = std::max(fzcap, sagecore::max_fragment_charge(p.max_fragment_charge, z) - 1);
    }
    return fzcap;
}

// Score.matched_b / matched_y are u16 in the reference (scoring.rs:21-22) and the rescoring kernel keeps the pair packed in one
// register (core.h: the `mm` counter): a peptide / charge combination that could match more than 65535 ions of one side would
// carry from one half into the other where the reference's release build wraps a u16 (and its debug build panics).  Refuse it:
// n-terminal resp. c-terminal ion kinds x ions per kind x fragment charges of the batch.
static int check_match_counters(const SageScorer* s, uint32_t fzcap) {
    const DevDbView& db = s->db->view;
    uint32_t nterm = 0;
    for (uint32_t k = 0; k < db.n_kinds; k++) nterm += db.ion_kinds[k] <= 2 ? 1u : 0u;
    const uint64_t per_kind = db.n_kinds ? s->db->max_ions / db.n_kinds : 0;  // (max_ions: ions of the longest peptide, all kinds)
    const uint64_t worst = std::max<uint64_t>(nterm, db.n_kinds - nterm) * per_kind * fzcap;
    if (worst > 65535)
        return fail(SAGE_HIP_ERR_UNSUPPORTED, "a candidate could match " + std::to_string(worst) + " ions of one terminus (" +
                                                  std::to_string(per_kind) + " ions per kind x fragment charges up to " + std::to_string(fzcap) +
                                                  "): beyond the u16 match counters of Score (scoring.rs:21-22)");
    return SAGE_HIP_OK;
}

// Spectra [c0, c1) of a host batch -> the device arrays of `d`, asynchronously on `up`:
//   * the per-spectrum arrays (40 bytes per spectrum) are staged through d's page-locked block (peak offsets rebased to the
//     range, the launch limits pcap / fzcap found on the way);
//   * the peak arrays go by DMA straight from the caller's memory when it is page-locked (sage_hip_host_alloc), else through
//     the staging block (copied by a few host threads).
// The caller must have waited for d->up_done before (the staging block is being rewritten).  `probe`: narrow-kernel variant.
static int stage_and_upload(SageScorer* s, SageDeviceBatch* d, const SageSpectrumBatch* b, uint32_t c0, uint32_t c1, bool peaks_locked,
                            const WindowEstimate& est, hipStream_t up, uint32_t sched_stride = SCHED_RECORD) {
    const uint32_t probe = est.probe;
    d->maybe_wide = est.maybe_wide;
    const uint32_t n = c1 - c0;
    const uint64_t base = n ? b->peak_off[c0] : 0, total = n ? b->peak_off[c1] - base : 0;
    if (n && b->peak_off[c1] < base) return fail(SAGE_HIP_ERR_INVALID, "peak_off is not monotone");
    const bool has_iso = b->isolation_lo && b->isolation_hi, has_rt = b->scan_start_time != nullptr,
               has_ims = b->inverse_ion_mobility != nullptr, has_fid = b->file_id != nullptr;
    d->n = n;
    HIP_TRY(d->masses.reserve(total));
    HIP_TRY(d->intensities.reserve(total));
    HIP_TRY(d->order.reserve(n));
    HIP_TRY(d->sort_a.reserve(n));
    HIP_TRY(d->sort_b.reserve(n));
    HIP_TRY(d->sort_idx.reserve(n));
    const size_t sort_bytes = schedule_temp_bytes(n);
    HIP_TRY(d->sort_tmp.reserve(sort_bytes));
    const bool use_sched = !getenv("SAGE_HIP_NO_SCHED");
    if (use_sched) { HIP_TRY(d->sched.reserve((size_t)sched_stride * n)); }
    const bool has_kind = has_iso && s->iso_kind != nullptr;
    const size_t small = ((size_t)n + 1) * 8 + (size_t)n * (4 * 7 + 1 + (has_kind ? 1 : 0)) + 64 * 13;
    HIP_TRY(d->stage.reserve(small + (peaks_locked ? 0 : total * 8 + 128)));
    HIP_TRY(d->meta.reserve(small));
    unsigned char* cur = d->stage.p;
    uint64_t* h_off = carve<uint64_t>(cur, (size_t)n + 1);
    float* h_mz = carve<float>(cur, n);
    uint8_t* h_z = carve<uint8_t>(cur, n);
    float* h_tic = carve<float>(cur, n);
    float* h_lo = has_iso ? carve<float>(cur, n) : nullptr;
    float* h_hi = has_iso ? carve<float>(cur, n) : nullptr;
    float* h_rt = has_rt ? carve<float>(cur, n) : nullptr;
    float* h_ims = has_ims ? carve<float>(cur, n) : nullptr;
    uint32_t* h_fid = has_fid ? carve<uint32_t>(cur, n) : nullptr;
    uint8_t* h_kind = has_kind ? carve<uint8_t>(cur, n) : nullptr;
    uint32_t pcap = 1, zmax = 0;
    bool any_unknown = false;
    h_off[0] = 0;
    // page-locked peak arrays go by DMA from where they lie: enqueued FIRST, so that the link is busy while this thread stages
    // the per-spectrum block below (0.3 ms per 131 072 spectra — at the head of a call nothing else hides it)
    const bool peaks_first = peaks_locked && n && total && b->masses && b->intensities;
    if (peaks_first) {
        HIP_TRY(hipMemcpyAsync(d->masses.p, b->masses + base, total * 4, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(d->intensities.p, b->intensities + base, total * 4, hipMemcpyHostToDevice, up));
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t a = b->peak_off[c0 + i], e = b->peak_off[c0 + i + 1];
        if (e < a) return fail(SAGE_HIP_ERR_INVALID, "peak_off is not monotone");
        h_off[i + 1] = e - base;
        pcap = std::max<uint32_t>(pcap, (uint32_t)std::min<uint64_t>(e - a, 0xFFFFFFFFull));
        const uint8_t z = b->precursor_charge[c0 + i];
        zmax = std::max<uint32_t>(zmax, z);
        any_unknown = any_unknown || z == 0;
    }
    if (n) {
        std::memcpy(h_mz, b->precursor_mz + c0, (size_t)n * 4);
        std::memcpy(h_z, b->precursor_charge + c0, n);
        std::memcpy(h_tic, b->total_ion_current + c0, (size_t)n * 4);
        if (has_iso) {
            std::memcpy(h_lo, b->isolation_lo + c0, (size_t)n * 4);
            std::memcpy(h_hi, b->isolation_hi + c0, (size_t)n * 4);
        }
        if (has_rt) std::memcpy(h_rt, b->scan_start_time + c0, (size_t)n * 4);
        if (has_ims) std::memcpy(h_ims, b->inverse_ion_mobility + c0, (size_t)n * 4);
        if (has_fid) std::memcpy(h_fid, b->file_id + c0, (size_t)n * 4);
        if (has_kind) std::memcpy(h_kind, s->iso_kind + c0, n);
    }
    const size_t meta_bytes = (size_t)(cur - d->stage.p);
    auto image = [&](const void* h) { return h ? d->meta.p + ((const unsigned char*)h - d->stage.p) : nullptr; };
    const float* src_m = b->masses ? b->masses + base : nullptr;
    const float* src_i = b->intensities ? b->intensities + base : nullptr;
    if (!peaks_locked && total) {
        float* h_m = carve<float>(cur, total);
        float* h_i = carve<float>(cur, total);
        const float *pm_ = src_m, *pi_ = src_i;
        parallel_for(total, 1u << 20, [&](size_t ib, size_t ie, unsigned) {
            std::memcpy(h_m + ib, pm_ + ib, (ie - ib) * 4);
            std::memcpy(h_i + ib, pi_ + ib, (ie - ib) * 4);
        });
        src_m = h_m;
        src_i = h_i;
    }
    if (n) {
        // the per-spectrum arrays: one copy of the staging block's head, the device pointers are its image
        // ... and the launch schedule (ascending neutral precursor mass) is sorted from it on the device, both on a stream of their
        // own WHILE the peaks cross the link on `up` (behind the uploads, on their stream, the sort's dozen small kernels left the
        // link idle for ~0.1 ms per chunk of the streaming pipeline).  (The previous users of this slot's buffers are done: every
        // caller has waited for the slot's last batch.)
        HIP_TRY(d->sort_done.create(false));
        HIP_TRY(hipMemcpyAsync(d->meta.p, d->stage.p, meta_bytes, hipMemcpyHostToDevice, s->side_stream));
        HIP_TRY((hipError_t)schedule_on_device(n, (const float*)image(h_mz), (const uint8_t*)image(h_z), s->params.min_precursor_charge,
                                               d->sort_a.p, d->sort_b.p, d->sort_idx.p, d->order.p, d->sort_tmp.p, sort_bytes, s->side_stream));
        if (use_sched)
            schedule_records_on_device(n, d->order.p, (const uint64_t*)image(h_off), (const float*)image(h_mz), (const uint8_t*)image(h_z),
                                       (const float*)image(h_lo), (const float*)image(h_hi), (const uint8_t*)image(h_kind), d->sched.p,
                                       sched_stride, s->side_stream);
        HIP_TRY(hipEventRecord(d->sort_done.e, s->side_stream));
        if (total && !peaks_first) {
            HIP_TRY(hipMemcpyAsync(d->masses.p, src_m, total * 4, hipMemcpyHostToDevice, up));
            HIP_TRY(hipMemcpyAsync(d->intensities.p, src_i, total * 4, hipMemcpyHostToDevice, up));
        }
        HIP_TRY(hipStreamWaitEvent(up, d->sort_done.e, 0));  // (`up_done` below stands for both)
    }
    HIP_TRY(hipEventRecord(d->up_done.e, up));
    DevBatchView& v = d->view;
    v = DevBatchView{};
    v.n = n;
    v.n_dev = nullptr;
    v.spec_base = c0;
    v.peak_off = (const uint64_t*)image(h_off);
    v.masses = d->masses.p;
    v.intensities = d->intensities.p;
    v.precursor_mz = (const float*)image(h_mz);
    v.precursor_charge = (const uint8_t*)image(h_z);
    v.isolation_lo = (const float*)image(h_lo);
    v.isolation_hi = (const float*)image(h_hi);
    v.iso_kind = (const uint8_t*)image(h_kind);
    v.tic = (const float*)image(h_tic);
    v.rt = (const float*)image(h_rt);
    v.ims = (const float*)image(h_ims);
    v.file_id = (const uint32_t*)image(h_fid);
    v.order = d->order.p;
    v.sched = use_sched && n ? d->sched.p : nullptr;
    v.sched_stride = sched_stride;
    v.probe = probe;
    v.pcap = pcap;
    v.fzcap = batch_fzcap(s->params, zmax, any_unknown);
    return check_match_counters(s, v.fzcap);
}

static int check_batch_args(const SageSpectrumBatch* b) {
    if (b->n_spectra && (!b->peak_off || !b->precursor_mz || !b->precursor_charge || !b->total_ion_current))
        return fail(SAGE_HIP_ERR_INVALID, "missing required spectrum arrays");
    const uint64_t total = b->n_spectra ? b->peak_off[b->n_spectra] - b->peak_off[0] : 0;
    if (total && (!b->masses || !b->intensities)) return fail(SAGE_HIP_ERR_INVALID, "missing peak arrays");
    return SAGE_HIP_OK;
}

// A resident batch knows EXACTLY whether any of its precursor windows exceeds the narrow kernel's slot capacity: one small
// kernel over its spectra behind the upload (window_max_kernel: the partition points of IndexedDatabase::query per query),
// four bytes back with the upload's synchronisation.  The sample-based estimate (choose_probe) said "maybe" for any batch that
// is dense where peptides are dense — e.g. the shard of a rank that owns the light end of the mass axis — and a "maybe" costs the
// step ten empty launches, the second part's overlap, and a longer host turn-around (round 5: 0.75 against 0.69 ms per 62 500
// C3 spectra).  The streaming pipeline keeps the estimate (it decides before the spectra are on the device).
// A device batch may be scored by any handle; the windows in its records hold for a scorer with the uploading handle's index,
// precursor tolerance, wide_window, isotope-error range, charge range and override only (every other scorer searches: plan_step).
static WindowKey window_key(const SageScorer* s) {
    WindowKey k;
    std::memset(&k, 0, sizeof k);  // (compared as bytes)
    k.db_serial = s->db->serial;
    k.precursor_tol.kind = s->dev.precursor_tol.kind;
    k.precursor_tol.lo = s->dev.precursor_tol.lo;
    k.precursor_tol.hi = s->dev.precursor_tol.hi;
    k.wide_window = s->dev.wide_window;
    k.min_precursor_charge = s->dev.min_precursor_charge;
    k.max_precursor_charge = s->dev.max_precursor_charge;
    k.override_precursor_charge = s->dev.override_precursor_charge;
    k.min_isotope_err = s->dev.min_isotope_err;
    k.max_isotope_err = s->dev.max_isotope_err;
    return k;
}
static int exact_window_check(SageScorer* s, SageDeviceBatch* d, hipStream_t st) {
    // (tests force the estimate's answer.  The records' third uint4 then stays unwritten — and unread: without a sched_key no
    // scorer is told that the records hold windows, plan_step)
    if (getenv("SAGE_HIP_ASSUME_NARROW") || d->n == 0) return SAGE_HIP_OK;
    HIP_TRY(s->win_max.reserve(1));
    HIP_TRY(hipMemsetAsync(s->win_max.p, 0, 4, st));
    // (... and the window of every spectrum's first query stays in its schedule record: kernels.hip, window_max_kernel)
    const bool keep_windows = d->view.sched && d->view.sched_stride == SCHED_RECORD_WINDOW;
    launch_window_max(s->dev, d->view, s->db->view.pep_mono, s->db->view.np, s->win_max.p, keep_windows ? d->sched.p : nullptr, st);
    HIP_TRY(hipGetLastError());
    uint32_t widest = 0;
    HIP_TRY(hipMemcpyAsync(&widest, s->win_max.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    d->maybe_wide = widest > s->dev.wcap;
    d->widest = widest;
    if (keep_windows) {
        d->win_key = window_key(s);
        d->view.sched_key = &d->win_key;
    }
    return SAGE_HIP_OK;
}

static int batch_upload(SageScorer* s, const SageSpectrumBatch* b, const uint8_t* iso_kind, SageDeviceBatch** out) {
    if (!s || !b || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    int rc = check_batch_args(b);
    if (rc != SAGE_HIP_OK) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    KindScope kinds(s, iso_kind);
    HIP_TRY(hipSetDevice(s->db->device));
    auto d = std::make_unique<SageDeviceBatch>();
    d->device = s->db->device;
    HIP_TRY(d->up_done.create(false));
    const uint32_t n = b->n_spectra;
    const WindowEstimate est = choose_probe(s, n, b->precursor_mz, b->precursor_charge, b->isolation_lo, b->isolation_hi, s->iso_kind);
    rc = stage_and_upload(s, d.get(), b, 0, n, is_page_locked(b->masses) && is_page_locked(b->intensities), est, s->up_stream, SCHED_RECORD_WINDOW);
    if (rc != SAGE_HIP_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s->up_stream));
    rc = exact_window_check(s, d.get(), s->up_stream);
    if (rc != SAGE_HIP_OK) return rc;
    *out = d.release();
    return SAGE_HIP_OK;
}

static int batch_process_upload(SageScorer* s, const SageRawBatch* raw, const uint8_t* iso_kind, uint64_t take_top_n, int deisotope,
                                float min_deisotope_mz, uint32_t min_peaks, SageDeviceBatch** out, uint32_t* out_npeaks) {
    if (!s || !raw || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    const uint32_t n = raw->n_spectra;
    if (n && (!raw->peak_off || !raw->precursor_mz || !raw->precursor_charge))
        return fail(SAGE_HIP_ERR_INVALID, "missing required spectrum arrays");
    if (take_top_n == 0 || take_top_n > 0xFFFFu) return fail(SAGE_HIP_ERR_INVALID, "take_top_n must be in [1, 65535]");
    std::lock_guard<std::mutex> lock(s->mu);
    KindScope kinds(s, iso_kind);
    HIP_TRY(hipSetDevice(s->db->device));
    auto d = std::make_unique<SageDeviceBatch>();
    d->device = s->db->device;
    HIP_TRY(d->up_done.create(false));
    ProcessScratch w;
    std::vector<uint32_t> counts;
    std::vector<uint64_t> off;
    Ctx cx;
    cx.stream = s->stream;
    if (!process_raw_on_device(cx, raw, take_top_n, deisotope, min_deisotope_mz, min_peaks, w, d->peak_off, d->masses, d->intensities, d->tic,
                               counts, off))
        return fail(cx.code, cx.err);
    if (out_npeaks) std::copy(counts.begin(), counts.end(), out_npeaks);
    uint32_t pcap = 1, zmax = 0;
    bool any_unknown = false;
    for (uint32_t i = 0; i < n; i++) {
        pcap = std::max(pcap, (uint32_t)(off[i + 1] - off[i]));
        zmax = std::max<uint32_t>(zmax, raw->precursor_charge[i]);
        any_unknown = any_unknown || raw->precursor_charge[i] == 0;
    }
    // precursor-side arrays and the launch schedule
    d->n = n;
    HIP_TRY(d->precursor_mz.upload(raw->precursor_mz, n));
    HIP_TRY(d->charge.upload(raw->precursor_charge, n));
    const bool has_iso = raw->isolation_lo && raw->isolation_hi;
    if (has_iso) {
        HIP_TRY(d->iso_lo.upload(raw->isolation_lo, n));
        HIP_TRY(d->iso_hi.upload(raw->isolation_hi, n));
    }
    const bool has_kind = has_iso && s->iso_kind != nullptr;
    if (has_kind) HIP_TRY(d->iso_kind.upload(s->iso_kind, n));
    if (raw->scan_start_time) HIP_TRY(d->rt.upload(raw->scan_start_time, n));
    if (raw->inverse_ion_mobility) HIP_TRY(d->ims.upload(raw->inverse_ion_mobility, n));
    if (raw->file_id) HIP_TRY(d->file_id.upload(raw->file_id, n));
    HIP_TRY(d->order.alloc(n));
    HIP_TRY(d->sort_a.alloc(n));
    HIP_TRY(d->sort_b.alloc(n));
    HIP_TRY(d->sort_idx.alloc(n));
    const size_t sort_bytes = schedule_temp_bytes(n);
    HIP_TRY(d->sort_tmp.alloc(sort_bytes));
    HIP_TRY((hipError_t)schedule_on_device(n, d->precursor_mz.p, d->charge.p, s->params.min_precursor_charge, d->sort_a.p, d->sort_b.p,
                                           d->sort_idx.p, d->order.p, d->sort_tmp.p, sort_bytes, s->stream));
    const bool use_sched = !getenv("SAGE_HIP_NO_SCHED");
    if (use_sched) {
        HIP_TRY(d->sched.alloc((size_t)SCHED_RECORD_WINDOW * n));
        schedule_records_on_device(n, d->order.p, d->peak_off.p, d->precursor_mz.p, d->charge.p, has_iso ? d->iso_lo.p : nullptr,
                                   has_iso ? d->iso_hi.p : nullptr, has_kind ? d->iso_kind.p : nullptr, d->sched.p, SCHED_RECORD_WINDOW, s->stream);
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    DevBatchView& v = d->view;
    v = DevBatchView{};
    v.n = n;
    v.peak_off = d->peak_off.p;
    v.masses = d->masses.p;
    v.intensities = d->intensities.p;
    v.precursor_mz = d->precursor_mz.p;
    v.precursor_charge = d->charge.p;
    v.isolation_lo = has_iso ? d->iso_lo.p : nullptr;
    v.isolation_hi = has_iso ? d->iso_hi.p : nullptr;
    v.iso_kind = has_kind ? d->iso_kind.p : nullptr;
    v.tic = d->tic.p;
    v.rt = raw->scan_start_time ? d->rt.p : nullptr;
    v.ims = raw->inverse_ion_mobility ? d->ims.p : nullptr;
    v.file_id = raw->file_id ? d->file_id.p : nullptr;
    v.order = d->order.p;
    v.sched = use_sched && n ? d->sched.p : nullptr;
    v.sched_stride = SCHED_RECORD_WINDOW;
    const WindowEstimate est = choose_probe(s, n, raw->precursor_mz, raw->precursor_charge, raw->isolation_lo, raw->isolation_hi, s->iso_kind);
    v.probe = est.probe;
    d->maybe_wide = est.maybe_wide;
    v.pcap = pcap;
    v.fzcap = batch_fzcap(s->params, zmax, any_unknown);
    if (int rc = check_match_counters(s, v.fzcap); rc != SAGE_HIP_OK) return rc;
    if (int rc = exact_window_check(s, d.get(), s->stream); rc != SAGE_HIP_OK) return rc;
    *out = d.release();
    return SAGE_HIP_OK;
}

int sage_hip_batch_download(SageDeviceBatch* b, uint64_t* peak_off, float* masses, float* intensities, float* tic) {
    if (!b || !peak_off) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    if (b->n) HIP_TRY(hipMemcpy(peak_off, b->view.peak_off, ((size_t)b->n + 1) * 8, hipMemcpyDeviceToHost));
    else peak_off[0] = 0;
    const uint64_t total = b->n ? peak_off[b->n] : 0;
    if (masses && total) HIP_TRY(hipMemcpy(masses, b->view.masses, total * 4, hipMemcpyDeviceToHost));
    if (intensities && total) HIP_TRY(hipMemcpy(intensities, b->view.intensities, total * 4, hipMemcpyDeviceToHost));
    if (tic && b->n) HIP_TRY(hipMemcpy(tic, b->view.tic, (size_t)b->n * 4, hipMemcpyDeviceToHost));
    return SAGE_HIP_OK;
}


void sage_hip_batch_free(SageDeviceBatch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    delete b;
}

// ---- scoring ---------------------------------------------------------------------------------------------------------------
static uint64_t arena_entries_for(const SageScorer* s, uint32_t n) {
    // 16 Ki entries = 64 KiB per spectrum on average + two 64 Ki-entry chunks per resident workgroup (each takes its arena space
    // a chunk at a time); an exhausted arena is detected, and the batch is then scored in smaller pieces
    uint64_t e = std::max<uint64_t>((uint64_t)n * 16384, 16ull << 20) + (uint64_t)std::min(n, std::max(s->tile_blocks, s->tile_blocks8)) * (2u << 16);
    e = std::min<uint64_t>(e, 0xFFFFFFF0ull);
    if (const char* v = getenv("SAGE_HIP_ARENA_MB")) e = std::min<uint64_t>((uint64_t)std::max(1, atoi(v)) << 18, 0xFFFFFFF0ull);
    return e;
}

// The scorer's narrow first pass may hand its lists over in rows by schedule position (DevWork::hand): the production kernels with a
// list and its header in one row of a word per lane.  (Which launches do: plan_step.)
static bool hand_rows_possible(const SageScorer* s) {
    return s->hand_rows && s->dev.kmax <= HAND_LIST_MAX && !s->dev.big_path && !s->fused && !s->one_launch && !s->exact_always;
}

// The device working set of a launch of n spectra.  `lane`: which of the scorer's two sets (the streaming pipeline's second compute
// lane never takes the large-window path, so it never owns that path's buffers — the candidate arena alone is 64 KiB per
// spectrum).  `wide`: the large-window kernels will be launched (lane 0 only).  `st`: the stream the kernels will run on.
static int ensure_work(SageScorer* s, uint32_t n, int lane, bool wide, hipStream_t st) {
    WorkSet& w = lane ? s->ws2 : s->ws;
    if (n > w.cap_n) {
        HIP_TRY(w.cand.reserve((size_t)n * s->dev.kmax + 64));  // (+ 64: rescore_kernel reads a full wavefront's worth of every row)
        HIP_TRY(w.cand_len.reserve(n));
        HIP_TRY(w.totals.reserve((size_t)n * 2));
        HIP_TRY(w.status.reserve(n));
        HIP_TRY(w.queue.reserve(n));
        HIP_TRY(w.retry.reserve(n));
        HIP_TRY(w.item_of.reserve(n));
        HIP_TRY(w.ready.reserve(n));
        // (no launch has the epoch 0.  On the stream of the kernels that read it: the scorer's streams do not synchronise with
        // the null stream, and a plain hipMemset could land after a producer's epoch store)
        HIP_TRY(hipMemsetAsync(w.ready.p, 0, (size_t)w.ready.n * 4, st));
        HIP_TRY(hipStreamSynchronize(st));  // (growth is rare; the parts of a resident step start on their own streams without waiting for this one)
        w.epoch = 0;
        w.cap_n = n;
    }
    if (s->fast_ties && n > w.cap_tie) {
        // (n rows of ~2 KB: 1 GB for a 500 000-spectrum resident batch.  The search does not need them — without the rows every
        // tie takes the exact retry pass — so running out of memory HERE switches fast ties off instead of failing the call.)
        const hipError_t e = w.cnt_store.reserve((size_t)n * s->cnt_stride);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            s->fast_ties = false;
        } else {
            HIP_TRY(e);
            w.cap_tie = n;
        }
    }
    if (!wide && hand_rows_possible(s) && n > w.cap_hand) {
        // (512 bytes per spectrum.  Like the count rows, the search does not need them: out of memory HERE keeps the arrays by spectrum)
        const hipError_t e = w.hand.reserve((size_t)n * HAND_ROW_WORDS);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            s->hand_rows = false;
        } else {
            HIP_TRY(e);
            // (zeroed once: a row no kernel of this scorer has written yet reads as an empty list, never as peptide indices)
            HIP_TRY(hipMemsetAsync(w.hand.p, 0, w.hand.bytes(), st));
            HIP_TRY(hipStreamSynchronize(st));
            w.cap_hand = n;
        }
    }
    if (wide && lane == 0 && n > w.cap_wide) {
        // large-window pipeline: per-query records, verbatim slots, replayed heaps, and the candidate arena
        HIP_TRY(w.qrec.reserve((size_t)n * s->qmax));
        HIP_TRY(w.seeds.reserve((size_t)n * s->qmax * s->kstride));
        HIP_TRY(w.qres.reserve((size_t)n * s->qmax * s->kstride));
        const uint64_t arena_entries = arena_entries_for(s, n);
        if (arena_entries > w.arena.n) HIP_TRY(w.arena.alloc(arena_entries));
        w.cap_wide = n;
    }
    return SAGE_HIP_OK;
}
// PSM counts always; a device-side record buffer only when the records do not go straight to the caller's page-locked array
static int ensure_out(SageScorer* s, OutSet& o, uint32_t n, bool need_features) {
    HIP_TRY(o.out_count.reserve(n));
    if (need_features) HIP_TRY(o.features.reserve((size_t)n * s->params.report_psms));
    return SAGE_HIP_OK;
}

static DevWork make_work(SageScorer* s, OutSet& o, int pass, int lane = 0) {
    DevWork w{};
    WorkSet& ws = lane ? s->ws2 : s->ws;
    w.cand = ws.cand.p;
    w.cand_len = ws.cand_len.p;
    w.totals = ws.totals.p;
    w.status = ws.status.p;
    w.n_deferred = o.counters.p + (size_t)pass * CTR_COUNT;
    w.queue = ws.queue.p;
    w.retry = ws.retry.p;
    w.item_of = ws.item_of.p;
    w.ready = ws.ready.p;
    w.epoch = ws.epoch;
    w.search_lag = s->search_lag;
    w.replay_split = s->replay_split;
    w.kstride = s->kstride;
    w.reuse = 0;
    w.arena_ptr = w.n_deferred + CTR_ARENA_PTR;
    w.cnt_store = nullptr;  // (plan_step switches the cheap ties on for the first pass of a production search)
    w.cnt_stride = s->cnt_stride;
    w.tile_blocks = s->tile_blocks;
    w.qrec = ws.qrec.p;
    w.seeds = ws.seeds.p;
    w.qres = ws.qres.p;
    w.arena = ws.arena.p;
    w.arena_cap = (uint32_t)ws.arena.n;
    w.qmax = s->qmax;
    w.tile_shift = s->db->view.tile_shift;
    w.dbg = s->dbg.p;
    return w;
}

enum { MODE_SCORE = 0,  // order-free trims, then the exact retry pass over the spectra whose reported ranks tie
       MODE_EXACT = 1,  // every trim replays bounded_min_heapify: one pass
       MODE_FAST = 2 }; // order-free trims only (quick_score: which peptides survive does not depend on heap layouts)

// What a caller asks of the kernels of one batch: the batch, the OutSet and the stream, and by name whatever differs from the values here.
struct StepRequest {
    DevBatchView view;
    OutSet* out;
    hipStream_t stream;
    StepRequest(const DevBatchView& v, OutSet& o, hipStream_t st) : view(v), out(&o), stream(st) {}
    int mode = MODE_SCORE;
    bool with_rescore = true;
    // where the PSM records go — device memory (null: the OutSet's buffer) or the device-side view of page-locked host memory
    SageFeature* rec = nullptr;
    // false skips the ten launches of the large-window path: the caller checks the queue counter afterwards and repeats the
    // batch with wide == true if the guess was wrong
    bool wide = true;
    // a part of a batch scored next to other parts (score_resident_locked): its queue / retry lists start at that offset of the
    // shared arrays, and the PSM counts of all parts go to one buffer (they are indexed by spectrum; null: the OutSet's)
    uint32_t list_off = 0;
    uint32_t* count_buf = nullptr;
    // which of the scorer's two working sets (a lane-1 batch never takes the large-window path: the replay kernels' side stream
    // is lane 0's)
    int lane = 0;
    uint32_t widest = 0xFFFFFFFFu;  // SageDeviceBatch::widest, where the batch knows it
};
// Which passes of a request are enqueued now (resident steps, score_resident_locked).
enum class Passes {
    Both,        // the first pass and, behind it, the exact retry pass
    FirstOnly,   // the exact retry pass is launched later if it turns out to have anything to do
    RetryOnly,   // that retry pass alone (the first pass of this very request has completed)
};
// What plan_step decided for a request: everything the launches take, and which of them there will be.
struct StepPlan {
    DevScorer sc1{}, sc2{};    // first pass, exact retry pass
    DevBatchView view{}, v2{}; // ... the retry pass walks the retry list, not the schedule
    DevWork w1{}, w2{};
    SageFeature* rec = nullptr;
    uint32_t* count_buf = nullptr;
    bool wide = false;        // the large-window kernels are launched (the request's, or any launch sequence but the production one)
    bool fused = false;       // SAGE_HIP_FUSED=1: narrow_kernel as the first pass, too
    bool one_launch = false;  // SAGE_HIP_ONE_LAUNCH=1: search_kernel as the first pass
    bool two_pass = false;    // the exact retry pass belongs to this request
    bool huge = false;        // the wide-list kernels keep their lists in WorkSet::hugebuf
    bool wing = false;        // tile_count_wing_kernel counts (its windows in WorkSet::winbuf)
    bool hand_on = false;     // the first pass hands its lists over in rows by schedule position (DevWork::hand)
    bool later = false;       // queue_kernel builds the large-window queue behind prelim_kernel (DevWork::queue_later)
};

// Decide the launches of one request — nothing here enqueues a kernel; the working set grows if it has to (ensure_work, which
// may wait for the stream), and the OutSet is told what collect will need.
//   MODE_SCORE with rescoring, the production path.  First pass, order-free trims: prelim_kernel scores the narrow windows and
//   queues the others; when `wide`, the large-window kernels take the queue; rescore_kernel reports every spectrum except those
//   whose reported ranks tie in hyperscore, which it lists.  Exact retry pass over that list, launched unconditionally — the
//   list and its COUNT live on the device (the first pass's CTR_RETRY counter), so no host round trip separates the passes, and
//   with no tied spectrum its blocks exit at once: narrow_kernel (matching with bounded_min_heapify replayed + rescoring, one
//   launch) reports the narrow ones and queues the others; when `wide`, the large-window kernels and rescore_kernel follow.
//   SAGE_HIP_FUSED=1: narrow_kernel as the first pass, too.
//   Other modes: preliminary kernel, large-window kernels, rescoring kernel.
static int plan_step(SageScorer* s, const StepRequest& rq, Passes passes, StepPlan& p) {
    OutSet& o = *rq.out;
    p.wide = rq.wide;
    if (rq.lane && p.wide) return fail(SAGE_HIP_ERR_INTERNAL, "large windows on the second working set");
    WorkSet& wset = rq.lane ? s->ws2 : s->ws;
    DevScorer sc = s->dev;
    if (p.wide && !s->sched_desc_forced) sc.xcd_chunk &= 0x7FFFFFFFu;  // (heaviest-first is the narrow search's default: scorer_init)
    DevBatchView& view = p.view;
    view = rq.view;
    {  // the records' windows are this scorer's only if they were computed from what it would compute them from
        const WindowKey mine = window_key(s);
        view.sched_win = view.sched && view.sched_stride == SCHED_RECORD_WINDOW && view.sched_key && std::memcmp(view.sched_key, &mine, sizeof mine) == 0;
    }
    // (the stream variant of the preliminary kernels keeps a window per (peak, fragment charge) in LDS, the probe variant the peak
    // masses only: a batch of very large spectra is probed whatever the estimate said)
    if (!view.probe && (size_t)view.fzcap * view.pcap * 8 > 48 * 1024) view.probe = 1;
    if (!view.probe) {  // (the stream variant reads the peptide-major fragment list, which an index keeps only once asked for)
        const int rc_pm = ensure_pm_frag(s->db);
        if (rc_pm != SAGE_HIP_OK) return rc_pm;
    }
    const bool production = rq.mode == MODE_SCORE && rq.with_rescore;
    p.fused = s->fused && production;
    if (!production) p.wide = true;
    int rc = ensure_work(s, view.n, rq.lane, p.wide, rq.stream);
    if (rc != SAGE_HIP_OK) return rc;
    rc = ensure_out(s, o, view.n, rq.rec == nullptr);
    if (rc != SAGE_HIP_OK) return rc;
    p.rec = rq.rec ? rq.rec : o.features.p;
    p.count_buf = rq.count_buf ? rq.count_buf : o.out_count.p;
    p.one_launch = production && !p.fused && s->one_launch;
    // Lists wider than a wavefront (report_psms > 32) live in LDS while they fit a compute unit's 160 KB; a configuration whose
    // lists, heaps or per-candidate arrays do not — report_psms in the hundreds x many precursor-window queries per spectrum,
    // report_psms beyond ~500, thousands of peaks on top — gets them in a global-memory workspace, a slice per workgroup of the
    // (then capped) grids.  Slower again, and never a refusal.
    p.huge = false;
    if (sc.big_path) {
        const size_t cap = (size_t)160 * 1024;
        p.huge = prelim_lds_bytes(sc, view) > cap || rescore_lds_bytes(sc, view, s->db->max_ions, true) > cap || assemble_lds_bytes(sc) > cap ||
               (size_t)s->kstride * 8 + 256 > cap || getenv("SAGE_HIP_FORCE_HUGE") != nullptr;  // (tests force the workspace on small lists)
    }
    const size_t lds_p = sc.big_path ? prelim_lds_bytes(sc, view, p.huge)
                                     : std::max(production ? std::max(narrow_lds_bytes(sc, view), p.one_launch ? search_lds_bytes(sc, view) : (size_t)0) : (size_t)0, prelim_lds_bytes(sc, view)),
                 lds_r = rescore_lds_bytes(sc, view, s->db->max_ions, true, p.huge);
    // the large-window count kernel keeps a window per (peak, fragment charge) in LDS next to a tile's counters; when that does not
    // fit a compute unit, the instance with the windows in global memory takes the batch (tile_count_wing_kernel)
    p.wing = p.wide && tile_lds_bytes(s->db->view, sc, view) > 160 * 1024;
    const size_t lds_t = p.wide ? tile_lds_bytes(s->db->view, sc, view, false, p.wing) : 0;
    // (every per-spectrum kernel may take a whole CU's LDS: spectrum_kernel_prepare / bigk_kernel_prepare at scorer creation)
    const size_t lds_cap = (size_t)160 * 1024;
    const size_t lds_a = sc.big_path && !p.huge ? assemble_lds_bytes(sc) : 0;
    if (lds_p > lds_cap || lds_r > lds_cap || lds_a > lds_cap || lds_t > 160 * 1024)
        return fail(SAGE_HIP_ERR_UNSUPPORTED,
                    sc.big_path ? "candidate lists too long for the LDS of a compute unit (report_psms x precursor-window queries per spectrum, or peaks x "
                                   "fragment charges): lower report_psms or narrow the charge / isotope-error ranges"
                                 : "spectrum too large for the LDS of a compute unit (~15 000 peaks per processed spectrum): lower max_peaks");
    if (p.huge) {
        // (a slice per workgroup of the capped grids — and a batch of fewer spectra launches fewer workgroups: ADVICE r05)
        // (the per-query kernels launch min(spectra x queries per spectrum, cap) workgroups, the per-spectrum ones fewer)
        const uint64_t blocks = std::max<uint64_t>((uint64_t)view.n * std::max<uint32_t>(s->qmax, 1u), 1u);
        const size_t need = (size_t)std::min<uint64_t>(huge_grid(), blocks) * huge_stride_bytes(sc);
        if (wset.hugebuf.n < need) {
            HIP_TRY(hipStreamSynchronize(rq.stream));
            HIP_TRY(wset.hugebuf.reserve(need));
        }
    }
    if (p.wing) {  // [tile_blocks][2][fzcap * pcap] floats
        const size_t need = (size_t)std::max(s->tile_blocks, s->tile_blocks8) * 2 * view.fzcap * view.pcap;
        if (wset.winbuf.n < need) {
            HIP_TRY(hipStreamSynchronize(rq.stream));
            HIP_TRY(wset.winbuf.reserve(need));
        }
    }
    p.two_pass = production && !(p.fused && !p.wide);  // (the fused first pass settles the ties of narrow spectra itself)
    o.two_pass = p.two_pass;
    o.with_rescore = rq.with_rescore;
    o.wide_launched = p.wide;
    DevBatchView& v2 = p.v2;
    v2 = view;
    v2.sched = nullptr;  // (the retry list is not the schedule)
    v2.sched_win = 0;
    v2.order = wset.retry.p + rq.list_off;  // filled by the rescoring kernel of the first pass, in no particular order
    v2.n_dev = o.counters.p + CTR_RETRY;
    if (p.one_launch && ++wset.epoch == 0) wset.epoch = 1;
    DevWork &w1 = p.w1, &w2 = p.w2;
    w1 = make_work(s, o, 0, rq.lane);
    w2 = make_work(s, o, 1, rq.lane);
    for (DevWork* w : {&w1, &w2}) {
        w->queue += rq.list_off;
        w->retry += rq.list_off;
    }
    const bool fast_ties = s->fast_ties && production && !p.fused && !p.one_launch && p.two_pass;
    if (fast_ties) {  // (each part of a step owns the rows / entries [list_off, list_off + n) of these arrays)
        w1.cnt_store = wset.cnt_store.p + (size_t)rq.list_off * s->cnt_stride;  // (rows by schedule position within the part)
    }
    // The first pass's hand-over in schedule order (DevWork::hand), one trip earlier for rescore_kernel: where the pass is
    // prelim_kernel then rescore_kernel and nothing else — no large-window kernels behind prelim_kernel (they write and read the
    // arrays by spectrum), schedule records to read the row beside, a list and its header in 64 words.  Every other launch sequence
    // — the retry pass, quick_score and initial_hits (not `production`), SAGE_HIP_NO_SCHED=1 — keeps the arrays by spectrum.
    p.hand_on = production && !p.fused && !p.one_launch && !p.wide && !p.huge && view.sched != nullptr && hand_rows_possible(s) &&
                         (uint64_t)rq.list_off + view.n <= wset.cap_hand;
    if (p.hand_on) w1.hand = wset.hand.p + (size_t)rq.list_off * HAND_ROW_WORDS;  // (rows by schedule position within the part)
    if (passes != Passes::RetryOnly) s->last_hand = p.hand_on;
    if (p.wing) w1.winbuf = w2.winbuf = wset.winbuf.p;
    if (p.huge) {
        w1.hugebuf = w2.hugebuf = wset.hugebuf.p;
        w1.huge_stride = w2.huge_stride = (uint32_t)huge_stride_bytes(sc);
    }
    if (production && s->cnt8 && !p.wing) {  // (only a pass that is followed by the retry pass may count in u8)
        w1.cnt8 = 1;
        w1.tile_blocks = s->tile_blocks8;
    }
    if (production && s->reuse_counts) {  // the retry pass replays from the first pass's counts, appending to the same arena
        w2.reuse = 1;
        w2.arena_ptr = w1.arena_ptr;
    }
    p.later = false;
    if (!p.fused && !p.one_launch) {
        // With the large-window kernels behind it the preliminary kernel may only MARK the spectra it hands over, one small kernel
        // building their queue in ascending precursor mass (DevWork::queue_later) — where the batch's windows are known to lie
        // within a few tiles (a wide-window / DIA search).  One returning atomic per spectrum on the queue's counter costs
        // ~11 ns each (2.3 ms of C5's step, where every spectrum is handed over), and neighbours in the sorted queue share their
        // tiles: C5 44.3 -> 43.2 ms.  Not for windows of dozens of tiles (an open search): there the count kernel runs 6 % SLOWER
        // behind ANY sorted or regularly permuted queue than behind the atomics' arrival order (C4 33.6 -> 35.8 ms of
        // tile_count8_kernel, the same binary: not understood) — scripts/experiments/r06_lab/RESULTS.md, r8e - r8m.
        // (the line between the two: 16 tiles — C5's widest window, charge 4 of a 12 Da isolation window, holds ~4 tiles' worth of
        // candidates, C4's +-500 Da ~55)
        p.later = p.wide && rq.widest <= (16u << s->db->view.tile_shift);
        if (const char* e = getenv("SAGE_HIP_QUEUE_LATER")) p.later = p.wide && atoi(e) != 0;  // (tests and experiments force either way)
        w1.queue_later = p.later ? 1u : 0u;
    }
    p.sc1 = p.sc2 = sc;
    p.sc1.exact = rq.mode == MODE_EXACT ? 1u : 0u;
    p.sc1.fast_log = p.two_pass ? 1u : 0u;  // (an undecided logarithm is settled by the retry pass: launch_rescore)
    p.sc2.exact = 1u;
    p.sc2.fast_log = 0u;
    o.timed = s->timed;  // (sage_hip_scorer_set_timing_interval)
    // (RetryOnly is the late launch behind a FirstOnly step: the flag stays set until collect_retry has read the pass's counters)
    if (passes != Passes::RetryOnly) o.retry_deferred = passes == Passes::FirstOnly && p.two_pass;
    return SAGE_HIP_OK;
}

// The first pass of a planned request on `st`, behind the reset of its counters — nothing here waits for the device.
// OutSet::launches: what SageTiming::n_launches reports of a pass, counted where the launches are — one for the preliminary (or
// fused, or search) kernel, four for the large-window path, one for the rescoring kernel; the retry pass alike with five for the
// large-window path and its rescoring kernel.  A nominal count, as it always was: queue_kernel and the further launches inside
// launch_prelim_tile (the large-window path is ten launches) are not in it.
static int enqueue_first_pass(SageScorer* s, const StepPlan& p, OutSet& o, hipStream_t st) {
    const SideStream side{s->side_stream, s->side_fork.e, s->side_join.e};
    o.launches[0] = o.launches[1] = 0;
    // (score_resident's epilogue kernel leaves the counters zeroed for the next step: one command less ahead of the first kernel)
    if (!o.counters_clean) HIP_TRY(hipMemsetAsync(o.counters.p, 0, 2 * CTR_COUNT * 4, st));
    o.counters_clean = false;
    if (o.timed) HIP_TRY(hipEventRecord(o.ev[0].e, st));
    if (p.fused)
        launch_narrow(s->db->view, p.sc1, p.view, p.w1, s->lnfact.p, (uint32_t)s->lnfact.n, p.rec, p.count_buf, st);
    else if (p.one_launch)
        launch_search(s->db->view, p.sc1, p.view, p.w1, s->lnfact.p, (uint32_t)s->lnfact.n, p.rec, p.count_buf, st);
    else {
        launch_prelim(s->db->view, p.sc1, p.view, p.w1, st);
        if (p.later) launch_queue(p.sc1, p.view, p.w1, st);
    }
    o.launches[0] += 1;
    HIP_TRY(hipGetLastError());  // (a failed launch must not let the kernels downstream of it run on stale records)
    if (p.wide) {
        launch_prelim_tile(s->db->view, p.sc1, p.view, p.w1, st, &side);
        o.launches[0] += 4;
        HIP_TRY(hipGetLastError());
    }
    if (o.timed) HIP_TRY(hipEventRecord(o.ev[1].e, st));
    if (o.with_rescore && (p.wide || !(p.fused || p.one_launch))) {  // (behind search_kernel / the fused kernel: only the spectra the large-window kernels assembled)
        s->last_rescore = rescore_instance_code(p.sc1, p.w1, false);
        HIP_TRY((hipError_t)launch_rescore(s->db->view, p.sc1, p.view, p.w1, s->lnfact.p, (uint32_t)s->lnfact.n, s->db->max_ions, p.rec, p.count_buf, nullptr, st));
        o.launches[0] += 1;
    }
    if (o.timed) HIP_TRY(hipEventRecord(o.ev[2].e, st));
    return SAGE_HIP_OK;
}

// The exact retry pass of a planned request (StepPlan::two_pass) on `st`, behind ev[2].
static int enqueue_retry_pass(SageScorer* s, const StepPlan& p, OutSet& o, hipStream_t st) {
    const SideStream side{s->side_stream, s->side_fork.e, s->side_join.e};
    launch_narrow(s->db->view, p.sc2, p.v2, p.w2, s->lnfact.p, (uint32_t)s->lnfact.n, p.rec, p.count_buf, st);
    o.launches[1] += 1;
    HIP_TRY(hipGetLastError());
    if (p.wide) {
        launch_prelim_tile(s->db->view, p.sc2, p.v2, p.w2, st, &side);
        o.launches[1] += 4;
        HIP_TRY(hipGetLastError());
        // (without the large-window kernels the retry pass is ONE launch: no marker inside it)
        if (o.timed) HIP_TRY(hipEventRecord(o.ev[3].e, st));
        HIP_TRY((hipError_t)launch_rescore(s->db->view, p.sc2, p.v2, p.w2, s->lnfact.p, (uint32_t)s->lnfact.n, s->db->max_ions, p.rec, p.count_buf, nullptr, st));
        o.launches[1] += 1;
    }
    if (o.timed) HIP_TRY(hipEventRecord(o.ev[4].e, st));
    HIP_TRY(hipGetLastError());
    return SAGE_HIP_OK;
}

// Plan a request and enqueue its kernels on its stream: the first pass, and the retry pass behind it unless `passes` leaves it
// for later.  `plan` (may be null): what was decided, for a caller that launches more kernels on the same working set.
static int enqueue_step(SageScorer* s, const StepRequest& rq, Passes passes = Passes::Both, StepPlan* plan = nullptr) {
    StepPlan local;
    StepPlan& p = plan ? *plan : local;
    int rc = plan_step(s, rq, passes, p);
    if (rc != SAGE_HIP_OK) return rc;
    rc = enqueue_first_pass(s, p, *rq.out, rq.stream);
    if (rc != SAGE_HIP_OK) return rc;
    if (p.two_pass && passes == Passes::Both) return enqueue_retry_pass(s, p, *rq.out, rq.stream);
    HIP_TRY(hipGetLastError());
    return SAGE_HIP_OK;
}

// The retry pass that a Passes::FirstOnly request left out, launched after all: the same plan again, the retry list's length put
// back, the pass.
static int enqueue_late_retry(SageScorer* s, const StepRequest& rq) {
    OutSet& o = *rq.out;
    StepPlan p;
    const int rc = plan_step(s, rq, Passes::RetryOnly, p);
    if (rc != SAGE_HIP_OK) return rc;
    // the retry list's length: the first pass left it in the counter block, the epilogue sent it home and zeroed the block
    HIP_TRY(hipMemcpyAsync(o.counters.p + CTR_RETRY, o.h_counters + CTR_RETRY, 4, hipMemcpyHostToDevice, rq.stream));
    o.counters_clean = false;
    if (o.timed) HIP_TRY(hipEventRecord(o.ev[2].e, rq.stream));
    return enqueue_retry_pass(s, p, o, rq.stream);
}

// One pass's share of a step's figures (pass 0: the first, 1: the exact retry pass): its launches as the enqueuing function counted
// them and, where the launch recorded events, its kernel times — a preliminary, r rescoring (the retry pass: one figure, a, where
// the large-window kernels did not run).
static int add_pass(SageScorer* s, const OutSet& o, int pass) {
    SageTiming& t = s->timing;
    t.n_launches += o.launches[pass];
    if (!o.timed) return SAGE_HIP_OK;
    float a = 0, r = 0;
    if (pass == 0 || o.wide_launched) {
        HIP_TRY(hipEventElapsedTime(&a, o.ev[2 * pass].e, o.ev[2 * pass + 1].e));
        HIP_TRY(hipEventElapsedTime(&r, o.ev[2 * pass + 1].e, o.ev[2 * pass + 2].e));
    } else {
        HIP_TRY(hipEventElapsedTime(&a, o.ev[2].e, o.ev[4].e));
    }
    t.prelim_ms += a;
    t.rescore_ms += o.with_rescore ? r : 0.f;
    t.total_ms += a + (o.with_rescore ? r : 0.f);
    if (pass) t.retry_ms += a + r;
    return SAGE_HIP_OK;
}
// what a pass's overflow counters are refused with
static int arena_exhausted(const SageScorer* s) {
    return fail(SAGE_HIP_ERR_UNSUPPORTED, "large-window candidate arena exhausted (" + std::to_string(s->ws.arena.n >> 18) +
                                              " MiB): score this batch in smaller pieces or raise SAGE_HIP_ARENA_MB");
}
static int list_capacity_exceeded(uint32_t spectra) {
    return fail(SAGE_HIP_ERR_UNSUPPORTED, "preliminary candidate list capacity exceeded (" + std::to_string(spectra) + " spectra)");
}

// counters + timing of a finished batch (its comp_done / down_done event has completed); accumulates into s->timing.
// *redo_wide: the batch was launched without the large-window kernels and turned out to need them — nothing is accumulated.
static int collect(SageScorer* s, OutSet& o, bool* arena_overflow, bool* redo_wide = nullptr) {
    const uint32_t* c1 = o.h_counters;
    const uint32_t* c2 = o.h_counters + CTR_COUNT;
    if (!o.wide_launched && c1[CTR_QUEUED]) {
        if (redo_wide) {
            *redo_wide = true;
            return SAGE_HIP_OK;
        }
        return fail(SAGE_HIP_ERR_INTERNAL, "spectra queued for the large-window kernels, which were not launched");
    }
    if (const int rc = add_pass(s, o, 0)) return rc;
    // (a deferred retry pass has not run: collect_retry adds its share if it does)
    if (o.two_pass && !o.retry_deferred)
        if (const int rc = add_pass(s, o, 1)) return rc;
    SageTiming& t = s->timing;
    t.n_wide += c1[CTR_QUEUED];
    t.arena_entries = std::max(t.arena_entries, std::max(c1[CTR_ARENA_PTR], c2[CTR_ARENA_PTR]));
    t.n_retry += o.two_pass ? c1[CTR_RETRY] : 0;
    t.n_tied += c1[CTR_TIED];
    for (uint32_t k = 0; k < CTR_TIE_STRIPES; k++) t.n_tied += c1[CTR_TIE_STRIPE0 + k * CTR_TIE_STRIDE];
    if (c1[CTR_ARENA_OVERFLOW] || c2[CTR_ARENA_OVERFLOW]) {
        if (arena_overflow) {
            *arena_overflow = true;
            return SAGE_HIP_OK;
        }
        return arena_exhausted(s);
    }
    if (c1[CTR_LIST_OVERFLOW] || c2[CTR_LIST_OVERFLOW]) return list_capacity_exceeded(c1[CTR_LIST_OVERFLOW] + c2[CTR_LIST_OVERFLOW]);
    return SAGE_HIP_OK;
}

// ... of a retry pass that was launched by itself, behind a first pass that has been collected (enqueue_late_retry)
static int collect_retry(SageScorer* s, OutSet& o) {
    o.retry_deferred = false;
    const uint32_t* c2 = o.h_counters + CTR_COUNT;
    if (const int rc = add_pass(s, o, 1)) return rc;
    SageTiming& t = s->timing;
    t.arena_entries = std::max(t.arena_entries, c2[CTR_ARENA_PTR]);
    if (c2[CTR_ARENA_OVERFLOW]) return arena_exhausted(s);
    if (c2[CTR_LIST_OVERFLOW]) return list_capacity_exceeded(c2[CTR_LIST_OVERFLOW]);
    return SAGE_HIP_OK;
}

static void reset_timing(SageScorer* s) { s->timing = SageTiming{}; }

// Wait for a stream by polling first: a blocked hipStreamSynchronize wakes up tens of microseconds after the last command — a
// twentieth of a small step.  (Bounded: a long wait falls back to the blocking call.)
static hipError_t wait_for_stream(hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) return hipStreamSynchronize(st);
    }
}

// ---- resident steps --------------------------------------------------------------------------------------------------------
// SAGE_HIP_STEP_TRACE=1: host-side clock of a resident step on stderr (microseconds since the call began, and since the
// previous call returned) — where the host's share of a small step goes (scripts/experiments/r05_lab/gpu_r5i.sh)
struct StepTrace {
    using Clock = std::chrono::steady_clock;
    const bool on;
    const Clock::time_point enter = Clock::now();
    double enq = 0, wait = 0;  // the step's last command enqueued, its kernels done
    explicit StepTrace(bool on_) : on(on_) {}
    double us() const { return std::chrono::duration<double, std::micro>(Clock::now() - enter).count(); }
    ~StepTrace() {
        if (!on) return;
        static thread_local Clock::time_point prev_exit{};
        const auto now = Clock::now();
        fprintf(stderr, "[sage_hip] step: %.1f us since the previous call returned; enqueued at %.1f, kernels done at %.1f, returns at %.1f\n",
                std::chrono::duration<double, std::micro>(enter - prev_exit).count(), enq, wait,
                std::chrono::duration<double, std::micro>(now - enter).count());
        prev_exit = now;
    }
};

// the stream of part `wy` of a resident step (and of lane `wy` of the streaming pipeline)
static hipStream_t part_stream(const SageScorer* s, uint32_t wy) { return wy ? s->way_stream[wy - 1] : s->stream; }

// Wait for the streams of parts [0, k), the first parts first (they were launched first); every one of them is waited for
// whatever the others report.
static hipError_t wait_for_parts(const SageScorer* s, uint32_t k) {
    hipError_t first = hipSuccess;
    for (uint32_t wy = 0; wy < k; wy++) {
        const hipError_t e = wait_for_stream(part_stream(s, wy));
        if (first == hipSuccess) first = e;
    }
    return first;
}

// Part `wy` of `ways` of a resident batch as a request: its slice of the launch schedule (consecutive precursor masses), its start
// in the arrays the parts share, its stream and its OutSet.  What differs between the passes is the caller's to fill in.
static StepRequest part_request(SageScorer* s, const SageDeviceBatch* b, uint32_t wy, uint32_t ways, SageFeature* rec) {
    const uint32_t start = (uint32_t)((uint64_t)b->n * wy / ways), end = (uint32_t)((uint64_t)b->n * (wy + 1) / ways);
    StepRequest rq(b->view, s->outs[wy], part_stream(s, wy));
    rq.view.order += start;
    if (rq.view.sched) rq.view.sched += (size_t)rq.view.sched_stride * start;
    rq.view.n = end - start;
    rq.list_off = start;
    rq.rec = rec;
    return rq;
}

// A part's PSM counts — `counts`, unless the kernels stored them home already — and its counters in one launch, straight into the
// page-locked destinations
static int launch_part_epilogue(const StepRequest& part, const uint32_t* counts, bool counts_home, uint32_t* count_view, const uint32_t* order) {
    EpilogueParts parts{};
    parts.n = 1;
    parts.src[0] = part.out->counters.p;
    parts.dst[0] = part.out->h_counters_view;
    launch_epilogue(counts, counts_home ? 0u : part.view.n, count_view, order, parts, part.stream);
    HIP_TRY(hipGetLastError());
    return SAGE_HIP_OK;
}

// The retry pass after all, behind a step whose parts left it out and have been collected: the parts that have something to
// retry, each on its stream, and a second (short) wait.
static int launch_deferred_retries(SageScorer* s, const SageDeviceBatch* b, uint32_t ways, SageFeature* rec, uint32_t* count_view) {
    uint32_t launched = 0;
    for (uint32_t wy = 0; wy < ways; wy++) {
        if (s->outs[wy].h_counters[CTR_RETRY] == 0) {
            s->outs[wy].retry_deferred = false;
            continue;
        }
        StepRequest part = part_request(s, b, wy, ways, rec);
        part.wide = false;
        part.count_buf = ways > 1 ? count_view : s->outs[0].out_count.p;
        int rc = enqueue_late_retry(s, part);
        if (rc != SAGE_HIP_OK) {
            (void)wait_for_parts(s, ways);
            return rc;
        }
        rc = launch_part_epilogue(part, s->outs[0].out_count.p, part.count_buf == count_view, count_view, nullptr);
        if (rc != SAGE_HIP_OK) return rc;
        launched++;
    }
    if (!launched) return SAGE_HIP_OK;
    HIP_TRY(wait_for_parts(s, ways));
    for (uint32_t wy = 0; wy < ways; wy++) {
        OutSet& ow = s->outs[wy];
        ow.counters_clean = true;
        if (!ow.retry_deferred) continue;
        const int rc = collect_retry(s, ow);
        if (rc != SAGE_HIP_OK) return rc;
    }
    return SAGE_HIP_OK;
}

// What a finished step of `ways` parts reports of its time: total_ms is the first part's start to the LATEST end.
static int roll_up_timing(SageScorer* s, uint32_t ways) {
    if (s->timed) {
        float wall = 0.f;
        for (uint32_t wy = 0; wy < ways; wy++) {
            float w1 = 0.f;
            HIP_TRY(hipEventElapsedTime(&w1, s->way_begin.e, s->way_end[wy].e));
            wall = std::max(wall, w1);
        }
        s->timing.total_ms = wall;  // (prelim_ms / rescore_ms: summed over the parts, which overlap in time)
        s->kept_prelim_ms = s->timing.prelim_ms;
        s->kept_rescore_ms = s->timing.rescore_ms;
        s->kept_retry_ms = s->timing.retry_ms;
    } else {  // (an untimed step reports the kernel times of the last timed one; total_ms 0 says so)
        s->timing.prelim_ms = s->kept_prelim_ms;
        s->timing.rescore_ms = s->kept_rescore_ms;
        s->timing.retry_ms = s->kept_retry_ms;
        s->timing.total_ms = 0.f;
    }
    s->timing.n_ways = ways;
    return SAGE_HIP_OK;
}

// One attempt at a resident step: kernels, record download, ONE host synchronisation (a second, short one where a deferred
// retry pass is launched after all).  *needs_wide: the batch was launched without the large-window kernels and turned out to
// need them — nothing was accumulated, and no OutSet is left waiting for a retry pass.
static int resident_attempt(SageScorer* s, SageDeviceBatch* b, SageFeature* out, uint32_t* out_count, SageFeature* direct, StepTrace& trace,
                            bool* needs_wide) {
    *needs_wide = false;
    OutSet& o = s->outs[0];
    // A narrow-search batch in `ways` parts of the launch schedule (consecutive precursor masses), each on its own stream:
    // a part's kernels fill the GPU while another part's kernel starts cold, drains, or waits on the few wavefronts of its
    // retry pass.  Large-window batches go as one (their steps are long; the parts would fight over the candidate arena).
    // Default (no SAGE_HIP_WAYS): two parts for batches up to 196 608 spectra — the shards of a rank of a 3- to 8-GPU
    // strong-scaling run — where a good part of the step is cold starts, tails and the retry pass's handful of wavefronts (C3,
    // 62 500 spectra: -6 %; 125 000 .. 170 000 with the heaviest-first schedule of round 6: -1 .. -1.6 %); one part above, where
    // the kernels' durations are what the roofline is held against.
    const uint32_t want = s->ways ? s->ways : (b->n <= 196608u ? 2u : 1u);
    const uint32_t ways = (!b->maybe_wide && !s->exact_always && b->n >= 8192u * want) ? want : 1u;
    // (sized for the whole batch: the parts of a step index the working set by spectrum and share outs[0]'s count buffer and,
    // if any, its record buffer)
    int rc = ensure_work(s, b->n, 0, b->maybe_wide || s->exact_always, s->stream);
    if (rc != SAGE_HIP_OK) return rc;
    rc = ensure_out(s, o, b->n, direct == nullptr);
    if (rc != SAGE_HIP_OK) return rc;
    SageFeature* const rec = direct ? direct : o.features.p;
    uint32_t* const count_view = s->zero_copy && b->n ? (uint32_t*)device_view_cached(out_count) : nullptr;
    const bool epilogue = count_view != nullptr;  // (page-locked count array: the small results go home in one launch)
    // The exact retry pass (spectra with equal hyperscores at a reported rank that the rescoring kernel could not settle itself,
    // undecided logarithms) is one more launch per part behind the rescoring kernel — ~10 us of a step's tail for a list that
    // is empty in most searches (C3, C3T: 0 of 500 000 spectra).  A narrow-search step whose predecessor had nothing to retry
    // does not launch it: the first pass's counters come home with the epilogue, and only if they name retries is the retry
    // pass launched then, behind a second (short) wait.  The first step of a scorer, and any step after one that did retry,
    // launches it unconditionally, as before.
    const bool defer_retry = epilogue && direct && !b->maybe_wide && !s->exact_always && !s->retry_likely && !s->fused && !s->one_launch;
    // No events between the parts' streams: every entry point of a scorer returns with its streams idle, so a part's
    // stream has nothing to wait for at the start (round 4 forked the parts off the first stream with an event: the second
    // part's first kernel started ~30 us after the first's), and at the end every part sends ITS counts and counters home
    // with its own epilogue launch, back to back with its last kernel, and the host waits for each stream in turn (round 4
    // joined the parts on one stream for a single epilogue: ~20 us of cross-stream wake-up behind the last kernel of every
    // step; profiles/r05_small_step_timeline.txt).
    for (uint32_t wy = 0; wy < ways; wy++) {
        StepRequest part = part_request(s, b, wy, ways, rec);
        if (wy == 0 && s->timed) HIP_TRY(hipEventRecord(s->way_begin.e, part.stream));  // (SageTiming::total_ms: first part's start to last part's end)
        // the PSM counts: a step in parts has its kernels store them straight into the caller's page-locked array, as they do
        // the records (4-byte stores spread over the kernels' lifetime cost nothing there; a part's counts are scattered over
        // the array — its spectra are a range of the launch SCHEDULE — and gathering them at the end of the step costs 33 us of
        // scattered stores across the link, joining the parts for one contiguous copy 20 us of cross-stream wake-up:
        // profiles/r05_small_step_timeline.txt); a step in one part keeps them on the device and sends them home in one
        // contiguous run behind its last kernel (round 13 had the kernels of a one-part step of 500 000 spectra store them home
        // too, to save that run's ~35 us: rescore_kernel took 0.2 ms longer — DESIGN.md 10)
        part.count_buf = (epilogue && ways > 1 && direct) ? count_view : o.out_count.p;
        part.mode = s->exact_always ? MODE_EXACT : MODE_SCORE;
        part.wide = b->maybe_wide;
        part.widest = b->widest;
        rc = enqueue_step(s, part, defer_retry ? Passes::FirstOnly : Passes::Both);
        if (rc != SAGE_HIP_OK) {
            (void)wait_for_parts(s, wy);
            return rc;
        }
        if (epilogue) {  // (counts_home: the kernels stored the counts there already)
            rc = launch_part_epilogue(part, o.out_count.p, part.count_buf == count_view, count_view, ways > 1 ? part.view.order : nullptr);
            if (rc != SAGE_HIP_OK) return rc;
        } else {
            HIP_TRY(hipMemcpyAsync(part.out->h_counters, part.out->counters.p, 2 * CTR_COUNT * 4, hipMemcpyDeviceToHost, part.stream));
        }
        // (every part's end: the parts run side by side and any of them may finish last — SageTiming::total_ms is the first
        // part's start to the LATEST end; round 5 recorded the last part's only and under-reported a step whose first part
        // outlasted it: ADVICE r05)
        if (s->timed) HIP_TRY(hipEventRecord(s->way_end[wy].e, part.stream));
    }
    const hipStream_t fin = part_stream(s, ways - 1);
    if (!epilogue && b->n) {
        HIP_TRY(wait_for_parts(s, ways - 1));
        HIP_TRY(hipMemcpyAsync(out_count, o.out_count.p, (size_t)b->n * 4, hipMemcpyDeviceToHost, fin));
    }
    if (b->n && !direct) {
        HIP_TRY(wait_for_parts(s, ways - 1));
        HIP_TRY(hipMemcpyAsync(out, o.features.p, (size_t)b->n * s->params.report_psms * sizeof(SageFeature), hipMemcpyDeviceToHost, fin));
    }
    trace.enq = trace.us();
    HIP_TRY(wait_for_parts(s, ways));
    trace.wait = trace.us();
    for (uint32_t wy = 0; wy < ways; wy++) {
        if (epilogue) s->outs[wy].counters_clean = true;  // (the part's epilogue kernel zeroed them)
        bool redo = false;
        rc = collect(s, s->outs[wy], nullptr, &redo);
        if (rc != SAGE_HIP_OK) return rc;
        *needs_wide = *needs_wide || redo;
    }
    if (*needs_wide) {
        for (uint32_t wy = 0; wy < ways; wy++) s->outs[wy].retry_deferred = false;
        return SAGE_HIP_OK;
    }
    if (defer_retry) {
        rc = launch_deferred_retries(s, b, ways, rec, count_view);
        if (rc != SAGE_HIP_OK) return rc;
    }
    s->retry_likely = s->timing.n_retry != 0;
    return roll_up_timing(s, ways);
}

// score a resident batch on the compute stream: kernels, record download, ONE host synchronisation.  Page-locked result
// arrays receive the records straight from the kernels (the stores cross PCIe while the other wavefronts compute: no download
// phase); pageable ones through the device buffer and a copy.
static int score_resident_locked(SageScorer* s, SageDeviceBatch* b, SageFeature* out, uint32_t* out_count) {
    if (b->device != s->db->device) return fail(SAGE_HIP_ERR_INVALID, "batch and scorer live on different devices");
    HIP_TRY(hipSetDevice(s->db->device));
    reset_timing(s);
    static const bool step_trace = getenv("SAGE_HIP_STEP_TRACE") != nullptr;
    StepTrace trace(step_trace);
    s->timed = s->timing_every != 0 && (s->timing_calls++ % s->timing_every) == 0;
    struct Restore {  // (the other entry points — streaming, quick_score, initial_hits — always record their events)
        SageScorer* s;
        ~Restore() { s->timed = true; }
    } restore{s};
    SageFeature* const direct = s->zero_copy && b->n ? (SageFeature*)device_view_cached(out) : nullptr;
    bool needs_wide = false;
    int rc = resident_attempt(s, b, out, out_count, direct, trace, &needs_wide);
    if (rc != SAGE_HIP_OK || !needs_wide) return rc;
    // a wrong guess: once more, in one part and with the large-window kernels
    reset_timing(s);
    b->maybe_wide = true;  // (and stays so: the batch holds large windows after all)
    rc = resident_attempt(s, b, out, out_count, direct, trace, &needs_wide);
    if (rc == SAGE_HIP_OK && needs_wide) return fail(SAGE_HIP_ERR_INTERNAL, "large-window queue not drained");
    return rc;
}

int sage_hip_score_resident(SageScorer* s, SageDeviceBatch* b, SageFeature* out, uint32_t* out_count) {
    if (!s || !b || !out || !out_count) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(s->mu);
    return score_resident_locked(s, b, out, out_count);
}

// Spectra [r0, r1) of a host batch through the three-stage pipeline: while chunk c is scored on the compute stream, chunk
// c + 1 is staged and uploaded on the copy stream and the PSM records of chunk c - 1 return on the download stream.  Mirrors the
// reference's reader -> processor -> search overlap (runner.rs:365-375, 450-461) at the PCIe boundary.
// `pending` (may be null): the window estimate is still being worked out on a helper thread — the first chunk is staged and its
// upload enqueued without it (neither needs it), then it is waited for and written into the chunk's view (`est` is updated).
static int score_range(SageScorer* s, const SageSpectrumBatch* b, uint32_t r0, uint32_t r1, SageFeature* out, uint32_t* out_count,
                       uint32_t chunk, bool peaks_locked, WindowEstimate& est, std::vector<std::pair<uint32_t, uint32_t>>& overflowed,
                       std::future<WindowEstimate>* pending = nullptr) {
    const uint32_t rp = s->params.report_psms;
    // page-locked result arrays (sage_hip_host_alloc) receive the records from the kernels' own stores; pageable ones through a
    // page-locked landing block per slot (an asynchronous copy into pageable memory would stall the pipeline)
    const bool out_locked = is_page_locked(out) && is_page_locked(out_count);
    SageFeature* const direct = s->zero_copy && out_locked ? (SageFeature*)device_view(out) : nullptr;
    const int mode = s->exact_always ? MODE_EXACT : MODE_SCORE;
    struct Pending {
        uint32_t c0, c1;
        int slot;
    };
    constexpr int NSLOT = 4;
    Pending pend[NSLOT];
    bool has[NSLOT] = {false, false, false, false};
    // SAGE_HIP_TIMING=1: host-side wall clock of the pipeline's steps on stderr (microseconds since the call began)
    static const bool trace_on = std::getenv("SAGE_HIP_TIMING") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    auto trace = [&](const char* what, int k_) {
        if (trace_on)
            fprintf(stderr, "[sage_hip] score_range %8.1f us  %s %d\n",
                    std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_begin).count(), what, k_);
    };
    // an error with chunks still in flight: nothing may keep writing into the caller's arrays after the call has returned
    auto bail = [&](int rc) -> int {
        (void)hipStreamSynchronize(s->up_stream);
        (void)hipStreamSynchronize(part_stream(s, 0));
        (void)hipStreamSynchronize(part_stream(s, 1));
        (void)hipStreamSynchronize(s->down_stream);
        return rc;
    };
#define HIP_TRY_BAIL(expr)                                                                  \
    do {                                                                                    \
        const hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) return bail(fail(SAGE_HIP_ERR_HIP, hipGetErrorString(e_)));   \
    } while (0)
    // kernels + the way home of the records of one chunk (its input is resident in s->slots[slot])
    // Two chunks of a batch WITHOUT large windows are scored side by side, chunk k on compute lane k & 1 (own stream, own working
    // set): the cold start, the tail and the retry chain of one chunk's kernels are filled by the other's (what two scorer
    // handles on two host threads do, §6 of DESIGN.md, here inside the pipeline).  With large windows: lane 0 only.
    auto lane_of = [&](int slot, bool wide) { return (!wide && mode == MODE_SCORE && s->two_lanes) ? (slot & 1) : 0; };
    auto launch = [&](int slot, uint32_t c0, uint32_t c1, bool wide) -> int {
        SageDeviceBatch& in = s->slots[slot];
        OutSet& o = s->outs[slot];
        const int lane = lane_of(slot, wide);
        hipStream_t cs = part_stream(s, (uint32_t)lane);
        HIP_TRY_BAIL(hipStreamWaitEvent(cs, in.up_done.e, 0));
        StepRequest rq(in.view, o, cs);
        rq.mode = mode;
        rq.rec = direct ? direct + (size_t)c0 * rp : nullptr;
        rq.wide = wide;
        rq.lane = lane;
        int rc = enqueue_step(s, rq);
        if (rc != SAGE_HIP_OK) return bail(rc);
        HIP_TRY_BAIL(hipEventRecord(o.comp_done.e, cs));
        // the next upload into this slot (chunk k + 4) is enqueued only after finish(slot) has waited for this chunk's
        // download, which itself follows its kernels: no device-side guard is needed for the input buffers
        HIP_TRY_BAIL(hipStreamWaitEvent(s->down_stream, o.comp_done.e, 0));
        HIP_TRY_BAIL(hipMemcpyAsync(o.h_counters, o.counters.p, 2 * CTR_COUNT * 4, hipMemcpyDeviceToHost, s->down_stream));
        SageFeature* dst_f = out + (size_t)c0 * rp;
        uint32_t* dst_c = out_count + c0;
        if (!out_locked) {
            const size_t fb = (((size_t)(c1 - c0) * rp * sizeof(SageFeature) + 63) / 64) * 64;
            const hipError_t e_ = o.h_out.reserve(fb + (size_t)(c1 - c0) * 4);
            if (e_ != hipSuccess) return bail(fail(SAGE_HIP_ERR_HIP, hipGetErrorString(e_)));
            dst_f = (SageFeature*)o.h_out.p;
            dst_c = (uint32_t*)(o.h_out.p + fb);
        }
        HIP_TRY_BAIL(hipMemcpyAsync(dst_c, o.out_count.p, (size_t)(c1 - c0) * 4, hipMemcpyDeviceToHost, s->down_stream));
        if (!direct)
            HIP_TRY_BAIL(hipMemcpyAsync(dst_f, o.features.p, (size_t)(c1 - c0) * rp * sizeof(SageFeature), hipMemcpyDeviceToHost, s->down_stream));
        HIP_TRY_BAIL(hipEventRecord(o.down_done.e, s->down_stream));
        return SAGE_HIP_OK;
    };
    auto finish = [&](int slot) -> int {
        if (!has[slot]) return SAGE_HIP_OK;
        has[slot] = false;
        OutSet& o = s->outs[slot];
        HIP_TRY_BAIL(hipEventSynchronize(o.down_done.e));
        bool ovf = false, redo = false;
        int rc = collect(s, o, &ovf, &redo);
        if (rc != SAGE_HIP_OK) return bail(rc);
        if (redo) {
            // the chunk held large windows although the sample said otherwise: once more with the large-window kernels (its
            // input is still resident; the working set is shared, so behind whatever the compute stream is doing now)
            est.maybe_wide = true;
            rc = launch(slot, pend[slot].c0, pend[slot].c1, true);
            if (rc != SAGE_HIP_OK) return rc;
            HIP_TRY_BAIL(hipEventSynchronize(o.down_done.e));
            rc = collect(s, o, &ovf, nullptr);
            if (rc != SAGE_HIP_OK) return bail(rc);
        }
        if (!out_locked) {
            const uint32_t c0 = pend[slot].c0, cn = pend[slot].c1 - pend[slot].c0;
            std::memcpy(out + (size_t)c0 * rp, o.h_out.p, (size_t)cn * rp * sizeof(SageFeature));
            std::memcpy(out_count + c0, o.h_out.p + (((size_t)cn * rp * sizeof(SageFeature) + 63) / 64) * 64, (size_t)cn * 4);
        }
        if (ovf) overflowed.push_back({pend[slot].c0, pend[slot].c1});
        return SAGE_HIP_OK;
    };
    // (pieces of equal size: short first and last pieces — the kernels start earlier, less is left when the link goes quiet — were
    // measured and lose, round 3: C3 44.5 against 46.9 M spectra/s; round 4, the last piece alone cut in 1/2, 1/4, 1/4 on the
    // faster kernels and with the schedule sort off the link: 46 against 54 M spectra/s)
    int k = 0;
    for (uint32_t c0 = r0; c0 < r1; c0 += chunk, k++) {
        const uint32_t c1 = (uint32_t)std::min<uint64_t>((uint64_t)c0 + chunk, r1);
        const int slot = k % NSLOT;
        trace("wait for slot of chunk", k);
        int rc = finish(slot);  // chunk k - 4 used this slot: its records are home, its buffers are free
        if (rc != SAGE_HIP_OK) return rc;
        trace("stage chunk", k);
        SageDeviceBatch& in = s->slots[slot];
        // (the uploads of chunk k - 4 finished long ago — its kernels ran — so the staging block may be rewritten)
        rc = stage_and_upload(s, &in, b, c0, c1, peaks_locked, est, s->up_stream);
        if (pending && pending->valid()) {  // (also on the error path: the helper thread reads the caller's arrays)
            est = pending->get();
            in.view.probe = est.probe;
            in.maybe_wide = est.maybe_wide;
            trace("window estimate joined", k);
        }
        if (rc != SAGE_HIP_OK) return bail(rc);
        trace("launch chunk", k);
        rc = launch(slot, c0, c1, est.maybe_wide);
        if (rc != SAGE_HIP_OK) return rc;
        trace("launched chunk", k);
        pend[slot] = Pending{c0, c1, slot};
        has[slot] = true;
    }
#undef HIP_TRY_BAIL
    // a working set (candidate lists, arena) is shared by the chunks of its lane: their kernels run in order on the lane's
    // stream, and a chunk's records leave through its own OutSet, so the next chunk's kernels may start while they are on the way
    trace("drain", k);
    for (int j = 0; j < NSLOT; j++) {  // oldest first
        const int rc = finish((k + j) % NSLOT);
        if (rc != SAGE_HIP_OK) return rc;
    }
    trace("done", k);
    return SAGE_HIP_OK;
}

static int score_batch(SageScorer* s, const SageSpectrumBatch* b, const uint8_t* iso_kind, SageFeature* out, uint32_t* out_count) {
    if (!s || !b || (b->n_spectra && (!out || !out_count))) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    int rc = check_batch_args(b);
    if (rc != SAGE_HIP_OK) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    KindScope kinds(s, iso_kind);
    HIP_TRY(hipSetDevice(s->db->device));
    reset_timing(s);
    const uint32_t n = b->n_spectra;
    if (n == 0) return SAGE_HIP_OK;
    const bool peaks_locked = is_page_locked(b->masses) && is_page_locked(b->intensities);
    // The window estimate (1 024 sampled spectra x two searches over the peptide masses: ~0.5 ms of cache misses on a 4.75 M
    // peptide list) runs on a helper thread while this one stages the first chunk and enqueues its upload, which need neither
    // of its answers; score_range joins it before the chunk's first launch.
    std::future<WindowEstimate> pending = std::async(std::launch::async, [s, n, b]() {
        return choose_probe(s, n, b->precursor_mz, b->precursor_charge, b->isolation_lo, b->isolation_hi, s->iso_kind);
    });
    WindowEstimate est{};
    est.probe = 1;
    est.maybe_wide = false;
    std::vector<std::pair<uint32_t, uint32_t>> todo, next;
    rc = score_range(s, b, 0, n, out, out_count, s->chunk, peaks_locked, est, todo, &pending);
    if (pending.valid()) est = pending.get();  // (score_range left before its first chunk: an error)
    if (rc != SAGE_HIP_OK) return rc;
    // chunks whose large-window candidates did not fit the arena: again in halves (the arena is sized for the chunk, so a
    // piece with the same arena and half the spectra has twice the room per spectrum)
    while (!todo.empty()) {
        next.clear();
        for (auto& r : todo) {
            const uint32_t len = r.second - r.first;
            if (len <= 1)
                return fail(SAGE_HIP_ERR_UNSUPPORTED, "large-window candidate arena exhausted by a single spectrum (" +
                                                          std::to_string(s->ws.arena.n >> 18) + " MiB): raise SAGE_HIP_ARENA_MB");
            rc = score_range(s, b, r.first, r.second, out, out_count, (len + 1) / 2, peaks_locked, est, next);
            if (rc != SAGE_HIP_OK) return rc;
        }
        todo.swap(next);
    }
    return SAGE_HIP_OK;
}


int sage_hip_quick_score_resident(SageScorer* s, SageDeviceBatch* b, int prefilter_low_memory, uint8_t* keep) {
    if (!s || !b || !keep) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    if (b->device != s->db->device) return fail(SAGE_HIP_ERR_INVALID, "batch and scorer live on different devices");
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->db->device));
    reset_timing(s);
    OutSet& o = s->outs[0];
    StepRequest rq(b->view, o, s->stream);
    rq.mode = MODE_FAST;  // Scorer::initial_hits
    rq.with_rescore = false;
    StepPlan plan;
    int rc = enqueue_step(s, rq, Passes::Both, &plan);
    if (rc != SAGE_HIP_OK) return rc;
    const uint64_t np = s->db->view.np;
    HIP_TRY(s->keep.reserve(np));
    HIP_TRY(hipMemsetAsync(s->keep.p, 0, std::max<uint64_t>(np, 1), s->stream));
    const DevWork& w = plan.w1;  // (the lists the first pass just filled, in the global workspace where the plan put them)
    if (prefilter_low_memory) {
        s->last_rescore = rescore_instance_code(s->dev, w, true);
        HIP_TRY((hipError_t)launch_rescore(s->db->view, s->dev, b->view, w, s->lnfact.p, (uint32_t)s->lnfact.n, s->db->max_ions, o.features.p,
                                           o.out_count.p, s->keep.p, s->stream));
    } else
        launch_quick_mark(s->dev, b->view, w, s->keep.p, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(o.h_counters, o.counters.p, 2 * CTR_COUNT * 4, hipMemcpyDeviceToHost, s->stream));
    std::vector<uint8_t> h(np);
    HIP_TRY(hipMemcpyAsync(h.data(), s->keep.p, np, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    rc = collect(s, o, nullptr);
    if (rc != SAGE_HIP_OK) return rc;
    for (uint64_t i = 0; i < np; i++) keep[i] |= h[i];
    return SAGE_HIP_OK;
}

int sage_hip_initial_hits(SageScorer* s, SageDeviceBatch* b, uint64_t* packed, uint32_t cap, uint32_t* len,
                          uint64_t* matched_peaks, uint64_t* scored_candidates) {
    if (!s || !b || !packed || !len) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    if (cap < s->dev.kmax) return fail(SAGE_HIP_ERR_INVALID, "cap must be >= max(50, 2*report_psms)");
    if (b->device != s->db->device) return fail(SAGE_HIP_ERR_INVALID, "batch and scorer live on different devices");
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->db->device));
    reset_timing(s);
    OutSet& o = s->outs[0];
    StepRequest rq(b->view, o, s->stream);
    rq.mode = MODE_EXACT;  // the reference's heap layouts
    rq.with_rescore = false;
    int rc = enqueue_step(s, rq);
    if (rc != SAGE_HIP_OK) return rc;
    HIP_TRY(hipMemcpyAsync(o.h_counters, o.counters.p, 2 * CTR_COUNT * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    rc = collect(s, o, nullptr);
    if (rc != SAGE_HIP_OK) return rc;
    const uint32_t n = b->n, kmax = s->dev.kmax;
    std::vector<uint64_t> c((size_t)n * kmax);
    std::vector<uint32_t> tot((size_t)n * 2), st(n);
    HIP_TRY(hipMemcpy(c.data(), s->ws.cand.p, c.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(len, s->ws.cand_len.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tot.data(), s->ws.totals.p, tot.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st.data(), s->ws.status.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        if (st[i] != ST_OK && st[i] != ST_OK_ORDERED) return fail(SAGE_HIP_ERR_UNSUPPORTED, "spectrum " + std::to_string(i) + ": status " + std::to_string(st[i]));
        for (uint32_t j = 0; j < len[i]; j++) packed[(size_t)i * cap + j] = c[(size_t)i * kmax + j];
        if (matched_peaks) matched_peaks[i] = tot[2 * i];
        if (scored_candidates) scored_candidates[i] = tot[2 * i + 1];
    }
    return SAGE_HIP_OK;
}

// debugging aid (not part of the drop-in surface): cumulative per-phase shader cycles, [4 kernels][8 phases]
int sage_hip_debug_phase_cycles(SageScorer* s, unsigned long long* out32) {
    if (!s || !out32) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    if (!s->dbg.p) return fail(SAGE_HIP_ERR_INVALID, "set SAGE_HIP_PHASE_CLOCKS=1 before creating the scorer");
    std::vector<unsigned long long> all((size_t)DBG_BLOCKS * 32);
    HIP_TRY(hipMemcpy(all.data(), s->dbg.p, all.size() * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < 32; k++) out32[k] = 0;
    for (size_t b = 0; b < DBG_BLOCKS; b++)
        for (int k = 0; k < 32; k++) out32[k] += all[b * 32 + k];
    return SAGE_HIP_OK;
}

// the sums over all rows of words [first_word, first_word + count) of the block behind the phase cycles (device_types.h: DBG_PRUNE_WORDS)
static int sum_dbg_words(SageScorer* s, uint32_t first_word, uint32_t count, unsigned long long* out) {
    if (!s || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    if (!s->dbg.p) return fail(SAGE_HIP_ERR_INVALID, "set SAGE_HIP_PHASE_CLOCKS=1 before creating the scorer");
    std::vector<unsigned long long> all((size_t)DBG_BLOCKS * DBG_PRUNE_WORDS);
    HIP_TRY(hipMemcpy(all.data(), s->dbg.p + (size_t)DBG_BLOCKS * 32, all.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < count; k++) out[k] = 0;
    for (size_t b = 0; b < DBG_BLOCKS; b++)
        for (uint32_t k = 0; k < count; k++) out[k] += all[b * DBG_PRUNE_WORDS + first_word + k];
    return SAGE_HIP_OK;
}

// debugging aid: what the rescoring prune dropped so far — candidates, their (ion, charge) items, scoring rounds that left early,
// rounds with a passing candidate beside pruned ones (kernels.hip: DBG_PRUNE_*)
int sage_hip_debug_prune_counters(SageScorer* s, unsigned long long* out4) { return sum_dbg_words(s, 0, 4, out4); }
// debugging aid: the trips of the bitmap filter in front of the prune (kernels.hip: DBG_FILTER_*) — 64-ion chunks that took the
// flat route, their trips of 8 ions, the trips of 4 ions the per-lane filter would have made of those chunks, and the trips of 4
// ions of the chunks that took the per-lane route
int sage_hip_debug_filter_counters(SageScorer* s, unsigned long long* out4) { return sum_dbg_words(s, 4, 4, out4); }

// debugging aid: the cooperative path behind the prune (kernels.hip: DBG_HEAVY_*) — chunks of heavy candidates the wavefront took
// together, and the (ion, charge) matches it added up for them
int sage_hip_debug_heavy_counters(SageScorer* s, unsigned long long* out2) { return sum_dbg_words(s, 8, 2, out2); }

// debugging aid: which route the chunks of sage_hip_debug_heavy_counters took (kernels.hip: DBG_HEAVY_ONE_TRIP / _PER_CHARGE) — all
// items in one lookup trip with the sums from LDS, or a trip per fragment charge with the sums by readlane
int sage_hip_debug_heavy_routes(SageScorer* s, unsigned long long* out2) { return sum_dbg_words(s, 10, 2, out2); }

// debugging aid: 1 if the last first pass this scorer enqueued handed its preliminary lists over in rows by schedule position
// (DevWork::hand), 0 if in the arrays by spectrum
int sage_hip_debug_handover_route(SageScorer* s, uint32_t* out) {
    if (!s || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    *out = s->last_hand ? 1u : 0u;
    return SAGE_HIP_OK;
}

// debugging aid: the instance of the rescoring kernels the first pass of the last scoring step (or the last quick_score) launched —
// SAGE_HIP_RESCORE_INST_* bits, SAGE_HIP_RESCORE_INST_NONE before the first
int sage_hip_debug_rescore_instance(SageScorer* s, uint32_t* out) {
    if (!s || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    static_assert(RESCORE_INST_CHIMERA == SAGE_HIP_RESCORE_INST_CHIMERA && RESCORE_INST_KINDS2 == SAGE_HIP_RESCORE_INST_KINDS2 &&
                      RESCORE_INST_FAST == SAGE_HIP_RESCORE_INST_FAST && RESCORE_INST_ACC == SAGE_HIP_RESCORE_INST_ACC &&
                      RESCORE_INST_PROF == SAGE_HIP_RESCORE_INST_PROF && RESCORE_INST_BIG == SAGE_HIP_RESCORE_INST_BIG &&
                      RESCORE_INST_NONE == SAGE_HIP_RESCORE_INST_NONE,
                  "include/sage_hip.h names the bits of device_types.h");
    *out = s->last_rescore;
    return SAGE_HIP_OK;
}


int sage_hip_host_alloc(uint64_t bytes, void** out) {
    if (!out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    if (void* d = device_view(*out)) {  // (device_view_cached's registry)
        std::lock_guard<std::mutex> lock(g_blocks_mu);
        g_blocks.push_back(HostBlock{(const unsigned char*)*out, (unsigned char*)d, (size_t)(bytes ? bytes : 1)});
    }
    return SAGE_HIP_OK;
}
void sage_hip_host_free(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lock(g_blocks_mu);
        for (size_t i = 0; i < g_blocks.size(); i++)
            if (g_blocks[i].host == (const unsigned char*)p) {
                g_blocks.erase(g_blocks.begin() + (long)i);
                break;
            }
    }
    (void)hipHostFree(p);
}

int sage_hip_scorer_set_timing_interval(SageScorer* s, uint32_t every) {
    if (!s) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(s->mu);
    s->timing_every = every;
    s->timing_calls = 0;
    return SAGE_HIP_OK;
}

int sage_hip_last_timing(const SageScorer* s, SageTiming* out) {
    if (!s || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    *out = s->timing;
    return SAGE_HIP_OK;
}

// Entry points with and without the per-spectrum isolation-window kinds (include/sage_hip.h)
int sage_hip_batch_upload(SageScorer* s, const SageSpectrumBatch* b, SageDeviceBatch** out) { return batch_upload(s, b, nullptr, out); }
int sage_hip_batch_upload_kinds(SageScorer* s, const SageSpectrumBatch* b, const uint8_t* iso_kind, SageDeviceBatch** out) {
    return batch_upload(s, b, iso_kind, out);
}
int sage_hip_batch_process_upload(SageScorer* s, const SageRawBatch* raw, uint64_t take_top_n, int deisotope, float min_deisotope_mz,
                                  uint32_t min_peaks, SageDeviceBatch** out, uint32_t* out_npeaks) {
    return batch_process_upload(s, raw, nullptr, take_top_n, deisotope, min_deisotope_mz, min_peaks, out, out_npeaks);
}
int sage_hip_batch_process_upload_kinds(SageScorer* s, const SageRawBatch* raw, const uint8_t* iso_kind, uint64_t take_top_n,
                                        int deisotope, float min_deisotope_mz, uint32_t min_peaks, SageDeviceBatch** out,
                                        uint32_t* out_npeaks) {
    return batch_process_upload(s, raw, iso_kind, take_top_n, deisotope, min_deisotope_mz, min_peaks, out, out_npeaks);
}
int sage_hip_score_batch(SageScorer* s, const SageSpectrumBatch* b, SageFeature* out, uint32_t* out_count) {
    return score_batch(s, b, nullptr, out, out_count);
}
int sage_hip_score_batch_kinds(SageScorer* s, const SageSpectrumBatch* b, const uint8_t* iso_kind, SageFeature* out,
                               uint32_t* out_count) {
    return score_batch(s, b, iso_kind, out, out_count);
}
}  // extern "C"
