// capi_psm.hip — the steps of the C ABI (include/sage_hip.h) over the PSMs a search reported: fragment annotation, scoring of
// candidate lists (positional isomers), site localisation.  Host code only (their kernels: kernels.hip); each step runs on the
// scorer's stream under its mutex, in the scratch of SageScorer::psm.
#include "capi_state.h"

// The features and counts of the batch's PSM slots, reserved and enqueued for upload: what every step's kernels read first.
static int upload_psms(SageScorer* s, uint32_t n, size_t slots, const SageFeature* features, const uint32_t* counts) {
    PsmScratch& w = s->psm;
    HIP_TRY(w.feats.reserve(slots));
    HIP_TRY(w.counts.reserve(n));
    HIP_TRY(hipMemcpyAsync(w.feats.p, features, slots * sizeof(SageFeature), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(w.counts.p, counts, (size_t)n * 4, hipMemcpyHostToDevice, s->stream));
    return SAGE_HIP_OK;
}

// ... and the candidate lists per slot, after check_candidate_lists has passed them (list: the spectra that have candidates)
static int upload_candidate_lists(SageScorer* s, size_t slots, uint64_t total, const std::vector<uint32_t>& list, const uint64_t* cand_off,
                                  const uint32_t* cand_pep, const uint8_t* cand_charge) {
    PsmScratch& w = s->psm;
    hipStream_t st = s->stream;
    HIP_TRY(w.cand_off.reserve(slots + 1));
    HIP_TRY(w.cand_list.reserve(list.size()));
    HIP_TRY(w.cand_pep.reserve(total));
    if (cand_charge) HIP_TRY(w.cand_charge.reserve(total));
    HIP_TRY(hipMemcpyAsync(w.cand_off.p, cand_off, (slots + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w.cand_list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w.cand_pep.p, cand_pep, total * 4, hipMemcpyHostToDevice, st));
    if (cand_charge) HIP_TRY(hipMemcpyAsync(w.cand_charge.p, cand_charge, total, hipMemcpyHostToDevice, st));
    return SAGE_HIP_OK;
}

extern "C" {

int sage_hip_annotate_resident(SageScorer* s, SageDeviceBatch* b, const SageFeature* features, const uint32_t* counts,
                               SageFragments* out) {
    if (!s || !b || !features || !counts || !out || !out->psm_off) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    if (b->device != s->db->device) return fail(SAGE_HIP_ERR_INVALID, "batch and scorer live on different devices");
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->db->device));
    const uint32_t n = b->n, rp = s->params.report_psms;
    const size_t slots = (size_t)n * rp;
    // a PSM's Fragments hold exactly matched_b + matched_y entries (scoring.rs:725-752) == Feature.matched_peaks
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t r = 0; r < rp; r++) {
            out->psm_off[(size_t)i * rp + r] = total;
            if (r < counts[i]) {
                if (features[(size_t)i * rp + r].peptide_idx >= s->db->view.np) return fail(SAGE_HIP_ERR_INVALID, "feature peptide_idx out of range");
                total += features[(size_t)i * rp + r].matched_peaks;
            }
        }
    out->psm_off[slots] = total;
    if (total > out->capacity) return fail(SAGE_HIP_ERR_INVALID, "SageFragments.capacity is smaller than the sum of matched_peaks");
    if (total && (!out->kinds || !out->charges || !out->fragment_ordinals || !out->intensities || !out->mz_calculated || !out->mz_experimental))
        return fail(SAGE_HIP_ERR_INVALID, "missing SageFragments arrays");
    if (n == 0 || total == 0) return SAGE_HIP_OK;
    PsmScratch& w = s->psm;
    hipStream_t st = s->stream;
    HIP_TRY(w.an_off.reserve(slots + 1));
    HIP_TRY(w.an_kinds.reserve(total));
    HIP_TRY(w.an_charges.reserve(total));
    HIP_TRY(w.an_ord.reserve(total));
    HIP_TRY(w.an_int.reserve(total));
    HIP_TRY(w.an_calc.reserve(total));
    HIP_TRY(w.an_exp.reserve(total));
    if (const int rc = upload_psms(s, n, slots, features, counts)) return rc;
    HIP_TRY(hipMemcpyAsync(w.an_off.p, out->psm_off, (slots + 1) * 8, hipMemcpyHostToDevice, st));
    DevFragments df{total, w.an_kinds.p, w.an_charges.p, w.an_ord.p, w.an_int.p, w.an_calc.p, w.an_exp.p};
    launch_annotate(s->db->view, s->dev, b->view, w.feats.p, w.counts.p, w.an_off.p, df, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out->kinds, w.an_kinds.p, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->charges, w.an_charges.p, total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->fragment_ordinals, w.an_ord.p, total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->intensities, w.an_int.p, total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->mz_calculated, w.an_calc.p, total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->mz_experimental, w.an_exp.p, total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SAGE_HIP_OK;
}

}  // extern "C"
// The argument rules of the calls that take candidate lists per PSM slot (sage_hip_score_candidates_resident,
// sage_hip_localise_resident): everything their kernels index with is checked here — bad input is an error, never a device
// fault.  total: the number of candidates (0: nothing to do); list: the spectra that have one.
static int check_candidate_lists(const std::string& who, const SageScorer* s, const SageDeviceBatch* b, const SageFeature* features,
                                 const uint32_t* counts, const uint64_t* cand_off, const uint32_t* cand_pep, const uint8_t* cand_charge,
                                 bool out_given, uint64_t& total, std::vector<uint32_t>& list) {
    const uint32_t n = b->n, rp = s->params.report_psms;
    const size_t slots = (size_t)n * rp;
    const uint64_t np = s->db->view.np;
    if (cand_off[0] != 0) return fail(SAGE_HIP_ERR_INVALID, who + ": cand_off[0] must be 0");
    for (size_t t = 0; t < slots; t++)
        if (cand_off[t + 1] < cand_off[t]) return fail(SAGE_HIP_ERR_INVALID, who + ": cand_off decreases at slot " + std::to_string(t));
    total = cand_off[slots];
    if (total == 0) return SAGE_HIP_OK;
    if (!features || !counts || !cand_pep || !out_given) return fail(SAGE_HIP_ERR_INVALID, who + ": null argument");
    for (uint32_t i = 0; i < n; i++) {
        const size_t s0 = (size_t)i * rp;
        if (cand_off[s0 + rp] == cand_off[s0]) continue;
        if (counts[i] > rp) return fail(SAGE_HIP_ERR_INVALID, who + ": counts[" + std::to_string(i) + "] exceeds report_psms");
        for (uint32_t r = 0; r < rp; r++) {
            if (r >= counts[i]) {
                if (cand_off[s0 + r + 1] != cand_off[s0 + r])
                    return fail(SAGE_HIP_ERR_INVALID, who + ": candidates on slot " + std::to_string(s0 + r) +
                                                          ", which holds no PSM (rank >= counts[" + std::to_string(i) + "])");
                continue;
            }
            const SageFeature& f = features[s0 + r];
            if (f.peptide_idx >= np) return fail(SAGE_HIP_ERR_INVALID, who + ": feature peptide_idx out of range");
            if (f.charge > 254) return fail(SAGE_HIP_ERR_INVALID, who + ": feature charge above 254");
        }
        list.push_back(i);
    }
    for (uint64_t c = 0; c < total; c++) {
        if (cand_pep[c] >= np)
            return fail(SAGE_HIP_ERR_INVALID, who + ": cand_pep[" + std::to_string(c) + "] is not a peptide of the database");
        if (cand_charge && cand_charge[c] > 254)
            return fail(SAGE_HIP_ERR_INVALID, who + ": cand_charge[" + std::to_string(c) + "] above 254");
    }
    return SAGE_HIP_OK;
}
extern "C" {

int sage_hip_score_candidates_resident(SageScorer* s, SageDeviceBatch* b, const SageFeature* features, const uint32_t* counts,
                                       const uint64_t* cand_off, const uint32_t* cand_pep, const uint8_t* cand_charge,
                                       SageCandidateScore* out) {
    if (!s || !b || !cand_off) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_score_candidates_resident: null argument");
    if (b->device != s->db->device) return fail(SAGE_HIP_ERR_INVALID, "batch and scorer live on different devices");
    std::lock_guard<std::mutex> lock(s->mu);
    const uint32_t n = b->n, rp = s->params.report_psms;
    const size_t slots = (size_t)n * rp;
    PsmScratch& w = s->psm;
    w.cs_call_ms = w.cs_kernel_ms = 0.f;
    uint64_t total = 0;
    std::vector<uint32_t> list;
    if (const int rc = check_candidate_lists("sage_hip_score_candidates_resident", s, b, features, counts, cand_off, cand_pep, cand_charge,
                                             out != nullptr, total, list))
        return rc;
    if (total == 0) return SAGE_HIP_OK;
    if (candidates_lds_bytes(b->view) > 160 * 1024)
        return fail(SAGE_HIP_ERR_UNSUPPORTED, "sage_hip_score_candidates_resident: a spectrum of the batch has more peaks than a compute unit's LDS holds");
    HIP_TRY(hipSetDevice(s->db->device));
    HIP_TRY(w.cs_ev.create());
    HIP_TRY(w.cs_out.reserve(total));
    hipStream_t st = s->stream;
    HIP_TRY(hipEventRecord(w.cs_ev[0], st));
    if (const int rc = upload_psms(s, n, slots, features, counts)) return rc;
    if (const int rc = upload_candidate_lists(s, slots, total, list, cand_off, cand_pep, cand_charge)) return rc;
    HIP_TRY(hipEventRecord(w.cs_ev[1], st));
    launch_candidates(s->db->view, s->dev, b->view, w.feats.p, w.counts.p, w.cand_list.p, (uint32_t)list.size(), w.cand_off.p,
                      w.cand_pep.p, cand_charge ? w.cand_charge.p : nullptr, s->lnfact.p, (uint32_t)s->lnfact.n, w.cs_out.p, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.cs_ev[2], st));
    HIP_TRY(hipMemcpyAsync(out, w.cs_out.p, total * sizeof(SageCandidateScore), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(w.cs_ev[3], st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&w.cs_call_ms, w.cs_ev[0], w.cs_ev[3]));
    HIP_TRY(hipEventElapsedTime(&w.cs_kernel_ms, w.cs_ev[1], w.cs_ev[2]));
    return SAGE_HIP_OK;
}
int sage_hip_last_candidates_timing(const SageScorer* s, float* call_ms, float* kernel_ms) {
    if (!s || !call_ms || !kernel_ms) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_last_candidates_timing: null argument");
    *call_ms = s->psm.cs_call_ms;
    *kernel_ms = s->psm.cs_kernel_ms;
    return SAGE_HIP_OK;
}

int sage_hip_ascore_from_counts(const uint16_t* n, uint32_t n_items, const uint16_t* a, const uint16_t* b, uint32_t n_site_items,
                                double* depth_scores, double* peptide_score_out, uint8_t* depth, double* ascore) {
    DepthScores ds;
    if (n) {
        for (int d = 0; d < 10; d++)
            if (n[d] > n_items) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_ascore_from_counts: a count exceeds n_items");
        if (depth_scores)
            for (uint32_t d = 1; d <= 10; d++) depth_scores[d - 1] = ds.get(n[d - 1], n_items, d);
        if (peptide_score_out) *peptide_score_out = peptide_score(ds, n, n_items);
    } else if (depth_scores || peptide_score_out) {
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_ascore_from_counts: depth_scores / peptide_score need n");
    }
    if (a || b || depth || ascore) {
        if (!a || !b || !depth || !ascore) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_ascore_from_counts: a, b, depth and ascore go together");
        for (int d = 0; d < 10; d++)
            if (a[d] > n_site_items || b[d] > n_site_items)
                return fail(SAGE_HIP_ERR_INVALID, "sage_hip_ascore_from_counts: a count exceeds n_site_items");
        *ascore = ascore_of(ds, a, b, n_site_items, *depth);
    }
    return SAGE_HIP_OK;
}

int sage_hip_localise_resident(SageScorer* s, SageDeviceBatch* b, const SageFeature* features, const uint32_t* counts,
                               const uint64_t* cand_off, const uint32_t* cand_pep, const uint8_t* cand_charge,
                               SageDepthCounts* per_candidate, SageLocalisation* per_slot) {
    const std::string who = "sage_hip_localise_resident";
    if (!s || !b || !cand_off) return fail(SAGE_HIP_ERR_INVALID, who + ": null argument");
    if (b->device != s->db->device) return fail(SAGE_HIP_ERR_INVALID, "batch and scorer live on different devices");
    std::lock_guard<std::mutex> lock(s->mu);
    const uint32_t n = b->n, rp = s->params.report_psms;
    const size_t slots = (size_t)n * rp;
    PsmScratch& w = s->psm;
    w.lc_call_ms = w.lc_kernel_ms = 0.f;
    uint64_t total = 0;
    std::vector<uint32_t> list;
    if (const int rc = check_candidate_lists(who, s, b, features, counts, cand_off, cand_pep, cand_charge, per_slot != nullptr, total, list))
        return rc;
    if (total == 0) return SAGE_HIP_OK;
    // the pair's items are compared position by position: one residue count and one number of fragment charges per slot
    const std::vector<uint16_t>& len = s->db->h_len;
    const uint32_t nk = s->db->view.n_kinds;
    for (uint32_t i : list)
        for (uint32_t r = 0; r < counts[i]; r++) {
            const size_t slot = (size_t)i * rp + r;
            uint32_t len0 = 0, nfz0 = 0;
            for (uint64_t c = cand_off[slot]; c < cand_off[slot + 1]; c++) {
                const uint32_t z = cand_charge && cand_charge[c] ? cand_charge[c] : features[slot].charge;
                const uint32_t nfz = sagecore::max_fragment_charge(s->dev.max_fragment_charge, z) - 1, l = len[cand_pep[c]];
                if (c == cand_off[slot]) {
                    len0 = l;
                    nfz0 = nfz;
                }
                if (l != len0 || nfz != nfz0)
                    return fail(SAGE_HIP_ERR_INVALID, who + ": the candidates of slot " + std::to_string(slot) +
                                                          " differ in residue count or in fragment charges (cand_pep[" + std::to_string(c) + "])");
                if ((uint64_t)nk * (l ? l - 1 : 0) * nfz > 65535)
                    return fail(SAGE_HIP_ERR_UNSUPPORTED, who + ": cand_pep[" + std::to_string(c) + "] has more than 65535 items");
            }
        }
    if (localise_lds_bytes(b->view) > 160 * 1024)
        return fail(SAGE_HIP_ERR_UNSUPPORTED, who + ": a spectrum of the batch has more peaks than a compute unit's LDS holds");
    std::vector<SageDepthCounts> own;
    if (!per_candidate) {
        own.resize(total);
        per_candidate = own.data();
    }
    HIP_TRY(hipSetDevice(s->db->device));
    HIP_TRY(w.lc_ev.create());
    HIP_TRY(w.lc_list2.reserve(list.size()));
    HIP_TRY(w.lc_counts.reserve(total));
    HIP_TRY(w.lc_pair_a.reserve(slots));
    HIP_TRY(w.lc_pair_b.reserve(slots));
    HIP_TRY(w.lc_site.reserve(slots));
    hipStream_t st = s->stream;
    HIP_TRY(hipEventRecord(w.lc_ev[0], st));
    if (const int rc = upload_psms(s, n, slots, features, counts)) return rc;
    if (const int rc = upload_candidate_lists(s, slots, total, list, cand_off, cand_pep, cand_charge)) return rc;
    HIP_TRY(hipEventRecord(w.lc_ev[1], st));
    launch_depth_counts(s->db->view, s->dev, b->view, w.feats.p, w.counts.p, w.cand_list.p, (uint32_t)list.size(), w.cand_off.p,
                        w.cand_pep.p, cand_charge ? w.cand_charge.p : nullptr, w.lc_counts.p, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.lc_ev[2], st));
    HIP_TRY(hipMemcpyAsync(per_candidate, w.lc_counts.p, total * sizeof(SageDepthCounts), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // best and second peptide score per slot: a plain f64 `>`, ties to the smaller position
    std::vector<uint32_t> pair_a(slots, LOC_NONE), pair_b(slots, LOC_NONE), list2;
    for (size_t slot = 0; slot < slots; slot++) {
        SageLocalisation& o = per_slot[slot];
        std::memset(&o, 0, sizeof o);
        o.best = o.second = LOC_NONE;
        o.ascore = std::nan("");
    }
    for (uint32_t i : list) {
        bool pairs = false;
        for (uint32_t r = 0; r < counts[i]; r++) {
            const size_t slot = (size_t)i * rp + r;
            const uint64_t c0 = cand_off[slot], c1 = cand_off[slot + 1];
            if (c1 == c0) continue;
            SageLocalisation& o = per_slot[slot];
            double ps1 = 0.0, ps2 = 0.0;
            uint32_t i1 = LOC_NONE, i2 = LOC_NONE;
            for (uint64_t c = c0; c < c1; c++) {
                const double ps = peptide_score(w.lc_scores, per_candidate[c].n, per_candidate[c].n_items);
                const uint32_t at = (uint32_t)(c - c0);
                if (i1 == LOC_NONE || ps > ps1) {
                    ps2 = ps1;
                    i2 = i1;
                    ps1 = ps;
                    i1 = at;
                } else if (i2 == LOC_NONE || ps > ps2) {
                    ps2 = ps;
                    i2 = at;
                }
            }
            o.best = i1;
            o.best_score = ps1;
            o.depth = 0;
            if (i2 != LOC_NONE) {
                o.second = i2;
                o.second_score = ps2;
                pair_a[slot] = i1;
                pair_b[slot] = i2;
                pairs = true;
            }
        }
        if (pairs) list2.push_back(i);
    }
    std::vector<DevSiteCounts> site(slots);
    if (!list2.empty()) {
        HIP_TRY(hipMemcpyAsync(w.lc_list2.p, list2.data(), list2.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.lc_pair_a.p, pair_a.data(), slots * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.lc_pair_b.p, pair_b.data(), slots * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(w.lc_site.p, 0, slots * sizeof(DevSiteCounts), st));
        HIP_TRY(hipEventRecord(w.lc_ev[3], st));
        launch_site_counts(s->db->view, s->dev, b->view, w.feats.p, w.counts.p, w.lc_list2.p, (uint32_t)list2.size(), w.cand_off.p,
                           w.cand_pep.p, cand_charge ? w.cand_charge.p : nullptr, w.lc_pair_a.p, w.lc_pair_b.p, w.lc_site.p, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(w.lc_ev[4], st));
        HIP_TRY(hipMemcpyAsync(site.data(), w.lc_site.p, slots * sizeof(DevSiteCounts), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipEventRecord(w.lc_ev[5], st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t slot = 0; slot < slots; slot++) {
        if (pair_b[slot] == LOC_NONE) continue;
        SageLocalisation& o = per_slot[slot];
        const DevSiteCounts& c = site[slot];
        o.n_site_items = c.n_site_items;
        for (int j = 0; j < 5; j++) {
            o.a[2 * j] = (uint16_t)(c.a[j] & 0xFFFFu);
            o.a[2 * j + 1] = (uint16_t)(c.a[j] >> 16);
            o.b[2 * j] = (uint16_t)(c.b[j] & 0xFFFFu);
            o.b[2 * j + 1] = (uint16_t)(c.b[j] >> 16);
        }
        o.ascore = ascore_of(w.lc_scores, o.a, o.b, o.n_site_items, o.depth);
    }
    HIP_TRY(hipEventElapsedTime(&w.lc_call_ms, w.lc_ev[0], w.lc_ev[5]));
    float k1 = 0.f, k2 = 0.f;
    HIP_TRY(hipEventElapsedTime(&k1, w.lc_ev[1], w.lc_ev[2]));
    if (!list2.empty()) HIP_TRY(hipEventElapsedTime(&k2, w.lc_ev[3], w.lc_ev[4]));
    w.lc_kernel_ms = k1 + k2;
    return SAGE_HIP_OK;
}
int sage_hip_last_localise_timing(const SageScorer* s, float* call_ms, float* kernel_ms) {
    if (!s || !call_ms || !kernel_ms) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_last_localise_timing: null argument");
    *call_ms = s->psm.lc_call_ms;
    *kernel_ms = s->psm.lc_kernel_ms;
    return SAGE_HIP_OK;
}

}  // extern "C"
