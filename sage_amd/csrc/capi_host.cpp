// capi_host.cpp — the entry points of the C ABI (include/sage_hip.h) that take no scorer: the error string, the FASTA database,
// the mzML / MGF readers, the writers, the group graph, and the thin entry points of the post-search stages.
#include "capi_state.h"
#include "purity.h"
#include "tmt_rollup.h"

static thread_local std::string g_last_error;

int sagehip::fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

// What every stage on the device refuses first: a machine without one, and (n: the stage's feature count, 0 where it sets no bound)
// more features than its 31-bit indices hold.
static int stage_guard(const char* who, uint64_t n) {
    if (sage_hip_device_count() <= 0) return fail(SAGE_HIP_ERR_NO_DEVICE, std::string(who) + ": no HIP device (there is no CPU fallback)");
    if (n >= (1ull << 31)) return fail(SAGE_HIP_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 features");
    return SAGE_HIP_OK;
}

extern "C" {

const char* sage_hip_last_error(void) { return g_last_error.c_str(); }
int sage_hip_abi_version(void) { return SAGE_HIP_ABI_VERSION; }
int sage_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// post-search rescoring (rescore.hip)
int sage_hip_rescore(int device, const SageRescoreInput* in, SageRescoreOutput* out) {
    if (!in || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_rescore: null argument");
    if (const int rc = stage_guard("sage_hip_rescore", in->n)) return rc;
    if (in->precursor_tol.kind != SAGE_TOL_PPM && in->precursor_tol.kind != SAGE_TOL_DA)
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_rescore: Pct tolerance should never be used on mz");  // linear_discriminant.rs:142
    out->passing_spectrum = out->passing_peptide = out->passing_protein = 0;
    out->lda_fitted = 0;
    out->device_ms = 0.0f;
    std::memset(out->coef, 0, sizeof(out->coef));
    if (in->n == 0) return SAGE_HIP_OK;
    if (!in->features || !in->peptide_key || !in->protein_key || !out->discriminant_score || !out->posterior_error ||
        !out->spectrum_q || !out->peptide_q || !out->protein_q)
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_rescore: null array");
    std::string err;
    const int rc = rescore_on_device(device, *in, *out, err);
    return rc == SAGE_HIP_OK ? rc : fail(rc, err);
}

// protein groups and picked protein-group FDR (protein_groups.hip, groups.cpp)
int sage_hip_protein_groups(int device, const SageHostDb* db, const SageGroupInput* in, SageGroupOutput* out) {
    if (!db || !in || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_protein_groups: null argument");
    if (const int rc = stage_guard("sage_hip_protein_groups", in->n)) return rc;
    out->strings = nullptr;
    out->n_strings = out->passing_protein_group = 0;
    out->n_groups = out->n_meta_peptides = out->cover_rounds = 0;
    out->device_ms = 0.0f;
    out->host_graph_ms = 0.0;
    if (in->n && (!in->features || !in->peptide_q || !in->discriminant_score || !out->num_protein_groups || !out->protein_group_q ||
                  !out->string_id))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_protein_groups: null array");
    std::unique_ptr<SageGroupStrings> table(new SageGroupStrings);
    if (in->n) {
        std::string err;
        const int rc = protein_groups_on_device(device, db->db, *in, *out, table->strings, err);
        if (rc != SAGE_HIP_OK) return fail(rc, err);
    }
    out->n_strings = table->strings.size();
    out->strings = table.release();
    return SAGE_HIP_OK;
}
const char* sage_hip_group_string(const SageGroupStrings* strings, uint64_t id) {
    return strings && id < strings->strings.size() ? strings->strings[id].c_str() : nullptr;
}
void sage_hip_group_strings_free(SageGroupStrings* strings) { delete strings; }

int sage_hip_group_graph_build(const SageHostDb* db, const uint32_t* peptides, uint64_t n, SageGroupGraph** out) {
    if (!db || !out || (n && !peptides)) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_group_graph_build: null argument");
    for (uint64_t i = 0; i < n; ++i)
        if (peptides[i] >= db->db.n_peptides() || (i && peptides[i] <= peptides[i - 1]))
            return fail(SAGE_HIP_ERR_INVALID, "sage_hip_group_graph_build: peptide indices must be in range, ascending and distinct");
    std::unique_ptr<SageGroupGraph> g(new SageGroupGraph);
    build_group_graph(db->db, NameIndex(db->db), peptides, n, g->g);
    *out = g.release();
    return SAGE_HIP_OK;
}
int sage_hip_group_graph_view(const SageGroupGraph* graph, SageGroupGraphView* out) {
    if (!graph || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_group_graph_view: null argument");
    const GroupGraph& g = graph->g;
    *out = SageGroupGraphView{(uint32_t)g.protein_name.size(), g.n_meta, g.n_groups(), (uint64_t)g.edge_group.size(),
                              g.protein_db_id.data(), g.protein_decoy.data(), g.group_off.data(), g.group_proteins.data(),
                              g.evidence_off.data(), g.evidence.data(), g.edge_group.data(), g.edge_meta.data()};
    return SAGE_HIP_OK;
}
void sage_hip_group_graph_free(SageGroupGraph* graph) { delete graph; }

int sage_hip_predict_rt(int device, const SageRtInput* in, SageRtOutput* out) {
    if (!in || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_predict_rt: null argument");
    if (const int rc = stage_guard("sage_hip_predict_rt", in->n)) return rc;
    out->rt_fitted = out->ims_fitted = 0;
    out->rt_r2 = out->ims_r2 = 0.0;
    out->device_ms = 0.0f;
    if (in->n_files == 0 && in->n) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_predict_rt: n_files == 0");
    if (in->n == 0) {
        for (uint32_t k = 0; out->alignments && k < in->n_files; ++k) out->alignments[k] = SageAlignment{k, 0.0f, 1.0f, 0.0f};
        return SAGE_HIP_OK;
    }
    if (!in->features || !in->seq_off || !in->seq || !in->monoisotopic || !out->spectrum_q || !out->aligned_rt ||
        !out->predicted_rt || !out->delta_rt_model || !out->predicted_ims || !out->delta_ims_model)
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_predict_rt: null array");
    std::string err;
    const int rc = predict_rt_on_device(device, *in, *out, err);
    return rc == SAGE_HIP_OK ? rc : fail(rc, err);
}

int sage_hip_lfq(int device, const SageLfqInput* in, SageLfqOutput* out) { return sage_hip_lfq_im(device, in, nullptr, out); }

int sage_hip_lfq_im(int device, const SageLfqInput* in, const SageLfqMobility* ms1_mobility, SageLfqOutput* out) {
    if (!in || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_lfq: null argument");
    if (const int rc = stage_guard("sage_hip_lfq", 0)) return rc;
    const SageLfqSettings& st = in->settings;
    if (st.min_charge < 1 || st.max_charge < st.min_charge)
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_lfq: precursor charge range must be [lo >= 1, hi >= lo]");
    if (st.peak_scoring < SAGE_LFQ_RETENTION_TIME || st.peak_scoring > SAGE_LFQ_HYBRID || (st.integration != SAGE_LFQ_APEX &&
                                                                                           st.integration != SAGE_LFQ_SUM))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_lfq: unknown peak_scoring / integration strategy");
    if ((in->n_features && (!in->features || !in->aligned_rt || !in->peptide_q)) || (in->n_files && !in->alignments) ||
        (in->n_ms1 && !in->ms1) || (in->n_peptides && (!in->carbon || !in->sulfur)))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_lfq: null array");
    if (out->cap && (!out->peptide_idx || !out->charge || !out->decoy || !out->has_peak || !out->peak_rt || !out->left ||
                     !out->right || !out->score || !out->spectral_angle || !out->q_value || (in->n_files && !out->areas)))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_lfq: null output array");
    for (uint32_t b = 0; b < in->n_ms1; ++b)
        if (in->ms1[b].n_spectra && (!in->ms1[b].peak_off || !in->ms1[b].mz || !in->ms1[b].intensities))
            return fail(SAGE_HIP_ERR_INVALID, "sage_hip_lfq: null MS1 array");
    std::string err;
    const int rc = lfq_on_device(device, *in, ms1_mobility, *out, err);
    return rc == SAGE_HIP_OK ? rc : fail(rc, err);
}

int sage_hip_write_lfq(const char* path, const SageHostDb* db, const SageLfqOutput* grids, const uint64_t* rows, uint64_t n_rows,
                       const char* const* filenames, uint32_t n_files) {
    if (!path || !db || !grids || (n_rows && !rows) || (n_files && !filenames))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_lfq: null argument");
    for (uint64_t r = 0; r < n_rows; ++r)
        if (rows[r] >= grids->n_grids || grids->peptide_idx[rows[r]] >= db->db.n_peptides())
            return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_lfq: row out of range");
    std::string err;
    if (!write_lfq(path, db->db, *grids, rows, n_rows, filenames, n_files, err)) return fail(SAGE_HIP_ERR_INVALID, err);
    return SAGE_HIP_OK;
}

int sage_hip_write_tmt(const char* path, const char* const* headers, uint32_t n_labels, uint64_t n_rows, const uint32_t* file_id,
                       const char* const* spec_ids, const float* ion_injection_time, const float* intensity,
                       const char* const* filenames, uint32_t n_files) {
    if (!path || (n_labels && !headers) || (n_rows && (!file_id || !spec_ids || !ion_injection_time || (n_labels && !intensity))) ||
        (n_files && !filenames))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_tmt: null argument");
    for (uint64_t r = 0; r < n_rows; ++r)
        if (file_id[r] >= n_files || !spec_ids[r]) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_tmt: file id out of range or null id");
    std::string err;
    if (!write_tmt(path, headers, n_labels, n_rows, file_id, spec_ids, ion_injection_time, intensity, filenames, n_files, err))
        return fail(SAGE_HIP_ERR_INVALID, err);
    return SAGE_HIP_OK;
}

// TMT reporter ions (tmt.hip)
int sage_hip_tmt(int device, const SageTmtInput* in, SageTmtOutput* out) {
    if (!in || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_tmt: null argument");
    if (const int rc = stage_guard("sage_hip_tmt", 0)) return rc;
    std::string err;
    const int rc = tmt_on_device(device, *in, *out, err);
    return rc == SAGE_HIP_OK ? rc : fail(rc, err);
}

// protein-level label-free quantification, MaxLFQ (protein_lfq.hip)
int sage_hip_protein_lfq(int device, const SageProteinLfqInput* in, SageProteinLfqOutput* out) {
    if (!in || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_protein_lfq: null argument");
    out->log_ms = out->median_ms = out->solve_ms = out->device_ms = 0.0f;
    out->n_batches = 0;
    if (in->n_files > 65535u) return fail(SAGE_HIP_ERR_UNSUPPORTED, "sage_hip_protein_lfq: more than 65535 files");
    if (in->n_rows && (!in->protein_of_row || (in->n_files && !in->areas)))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_protein_lfq: null input array");
    if (in->n_proteins == 0) {
        for (uint64_t r = 0; r < in->n_rows; ++r)
            if (in->protein_of_row[r] != 0xFFFFFFFFu)
                return fail(SAGE_HIP_ERR_INVALID, "sage_hip_protein_lfq: a protein id that is not below n_proteins (0)");
        return SAGE_HIP_OK;
    }
    if (!out->n_rows_used || !out->n_components || (in->n_files && (!out->log_abundance || !out->intensity || !out->component)))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_protein_lfq: null output array");
    if (in->n_rows == 0 || in->n_files == 0) {  // nothing to launch: no file of any protein is quantified
        const uint64_t nf = in->n_files, cells = (uint64_t)in->n_proteins * nf, pairs = nf ? in->n_proteins * (nf * (nf - 1) / 2) : 0;
        for (uint32_t p = 0; p < in->n_proteins; ++p) out->n_rows_used[p] = out->n_components[p] = 0;
        for (uint64_t r = 0; r < in->n_rows; ++r) {
            const uint32_t p = in->protein_of_row[r];
            if (p == 0xFFFFFFFFu) continue;
            if (p >= in->n_proteins) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_protein_lfq: a protein id that is not below n_proteins");
            ++out->n_rows_used[p];
        }
        for (uint64_t i = 0; i < cells; ++i) {
            out->log_abundance[i] = std::nan("");
            out->intensity[i] = 0.0;
            out->component[i] = 0xFFFFFFFFu;
        }
        for (uint64_t i = 0; i < pairs; ++i) {
            if (out->pair_median) out->pair_median[i] = std::nan("");
            if (out->pair_count) out->pair_count[i] = 0;
        }
        return SAGE_HIP_OK;
    }
    if (const int rc = stage_guard("sage_hip_protein_lfq", in->n_rows)) return rc;
    std::string err;
    const int rc = protein_lfq_on_device(device, *in, *out, err);
    return rc == SAGE_HIP_OK ? rc : fail(rc, err);
}

int sage_hip_write_protein_lfq(const char* path, const char* const* protein_names, uint32_t n_proteins, const uint32_t* rows,
                               uint32_t n_out, const SageProteinLfqOutput* result, const char* const* filenames, uint32_t n_files) {
    if (!path || !result || (n_out && (!rows || !protein_names || !result->n_rows_used || !result->n_components ||
                                       (n_files && !result->intensity))) || (n_files && !filenames))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_protein_lfq: null argument");
    for (uint32_t r = 0; r < n_out; ++r)
        if (rows[r] >= n_proteins || !protein_names[rows[r]])
            return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_protein_lfq: protein id out of range or null name");
    std::string err;
    if (!write_protein_lfq(path, protein_names, rows, n_out, *result, filenames, n_files, err)) return fail(SAGE_HIP_ERR_INVALID, err);
    return SAGE_HIP_OK;
}

// roll-up of TMT reporter intensities to groups (tmt_rollup.hip); every check comes before the device is touched
int sage_hip_tmt_rollup(int device, const SageTmtRollupInput* in, SageTmtRollupOutput* out) {
    const char* const who = "sage_hip_tmt_rollup";
    if (!in || !out) return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": null argument");
    out->n_used_rows = 0;
    out->n_long_groups = out->n_label_slabs = 0;
    out->norm_ms = out->summary_ms = out->device_ms = 0.0f;
    if (in->normalise != SAGE_TMT_NORMALISE_NONE && in->normalise != SAGE_TMT_NORMALISE_TOTAL)
        return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": unknown normalise " + std::to_string(in->normalise));
    if (in->summary != SAGE_TMT_SUMMARY_SUM && in->summary != SAGE_TMT_SUMMARY_MEDIAN)
        return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": unknown summary " + std::to_string(in->summary));
    if (in->n_labels > tmtroll::MAX_LABELS) return fail(SAGE_HIP_ERR_UNSUPPORTED, std::string(who) + ": more than 65535 channels");
    if (in->n_rows >= (1ull << 31)) return fail(SAGE_HIP_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 rows");
    if (in->n_rows && in->n_labels == 0) return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": n_labels == 0");
    if (in->n_rows && (!in->group_of_row || !in->intensity)) return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": null input array");
    bool any = false;
    for (uint64_t r = 0; r < in->n_rows; ++r) {
        const uint32_t g = in->group_of_row[r];
        if (g == tmtroll::NONE) continue;
        if (g >= in->n_groups)
            return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": group id " + std::to_string(g) + " of row " + std::to_string(r) +
                                                  " is not below n_groups");
        any = true;
    }
    if (in->n_groups == 0) return SAGE_HIP_OK;
    if (!out->n_rows_used || (in->n_labels && (!out->abundance || !out->log_abundance || !out->n_cells || !out->factor || !out->column_sum)))
        return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": null output array");
    if (!any) {  // nothing to launch: no group is quantified
        const uint64_t cells = (uint64_t)in->n_groups * in->n_labels;
        for (uint32_t g = 0; g < in->n_groups; ++g) out->n_rows_used[g] = 0;
        for (uint32_t k = 0; k < in->n_labels; ++k) {
            out->factor[k] = 1.0;
            out->column_sum[k] = 0.0;
        }
        for (uint64_t i = 0; i < cells; ++i) {
            out->abundance[i] = 0.0;
            out->log_abundance[i] = std::nan("");
            out->n_cells[i] = 0;
        }
        return SAGE_HIP_OK;
    }
    if (const int rc = stage_guard(who, in->n_rows)) return rc;
    std::string err;
    const int rc = tmt_rollup_on_device(device, *in, *out, err);
    return rc == SAGE_HIP_OK ? rc : fail(rc, err);
}

int sage_hip_write_tmt_rollup(const char* path, const char* first_header, const char* const* headers, uint32_t n_labels, uint64_t n_out,
                              const char* const* names, const uint32_t* plex, const uint32_t* n_psms, const uint32_t* n_peptides,
                              const double* abundance) {
    if (!path || !first_header || (n_labels && !headers) || (n_out && (!names || !plex || !n_psms || !n_peptides || (n_labels && !abundance))))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_tmt_rollup: null argument");
    for (uint32_t k = 0; k < n_labels; ++k)
        if (!headers[k]) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_tmt_rollup: null header");
    for (uint64_t r = 0; r < n_out; ++r)
        if (!names[r]) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_tmt_rollup: null name");
    std::string err;
    if (!write_tmt_rollup(path, first_header, headers, n_labels, n_out, names, plex, n_psms, n_peptides, abundance, err))
        return fail(SAGE_HIP_ERR_INVALID, err);
    return SAGE_HIP_OK;
}

// precursor purity of reported PSMs from MS1 scans (purity.hip); every check comes before the device is touched
int sage_hip_precursor_purity(int device, const SagePurityInput* in, SagePurityOutput* out) {
    const char* const who = "sage_hip_precursor_purity";
    if (!in || !out) return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": null argument");
    out->n_sorted_spectra = out->n_scanned_spectra = 0;
    out->upload_ms = out->kernel_ms = out->device_ms = 0.0f;
    const SagePuritySettings& st = in->settings;
    if (st.max_isotope > purity::MAX_ISOTOPE) return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": max_isotope above 16");
    if (!(st.ppm_tolerance >= 0.0f) || std::isinf(st.ppm_tolerance))
        return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": ppm_tolerance must be finite and not negative");
    if (in->n_queries == 0) return SAGE_HIP_OK;
    if (!in->ms1_index || !in->precursor_mz || !in->charge || (in->n_ms1 && !in->ms1) || !out->n_window || !out->n_matched || !out->total ||
        !out->matched || !out->below || !out->purity)
        return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": null array");
    uint64_t n_spectra = 0;
    for (uint32_t b = 0; b < in->n_ms1; ++b) {
        const SageRawBatch& r = in->ms1[b];
        n_spectra += r.n_spectra;
        if (!r.n_spectra) continue;
        if (!r.peak_off) return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": null MS1 array");
        for (uint32_t i = 0; i < r.n_spectra; ++i) {
            if (r.peak_off[i + 1] < r.peak_off[i]) return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": peak_off is not monotone");
            if (r.peak_off[i + 1] - r.peak_off[i] > (uint64_t)INT32_MAX)
                return fail(SAGE_HIP_ERR_UNSUPPORTED, std::string(who) + ": a spectrum of more than 2^31 - 1 peaks");
        }
        if (r.peak_off[r.n_spectra] && (!r.mz || !r.intensities)) return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": null MS1 array");
    }
    bool any = false;
    for (uint64_t i = 0; i < in->n_queries; ++i) {
        if (in->ms1_index[i] == purity::NO_MS1) continue;
        if (in->ms1_index[i] >= n_spectra) return fail(SAGE_HIP_ERR_INVALID, std::string(who) + ": an ms1_index that is not below the number of spectra");
        any = true;
    }
    if (any)
        if (const int rc = stage_guard(who, 0)) return rc;
    std::string err;
    const int rc = purity_on_device(device, *in, *out, err);  // (no query with a spectrum: fills the outputs, no device call)
    return rc == SAGE_HIP_OK ? rc : fail(rc, err);
}

int sage_hip_write_purity(const char* path, uint64_t n_rows, const uint64_t* psm_id, const uint32_t* file_id, const char* const* spec_ids,
                          const uint8_t* charge, const char* const* ms1_ids, const float* isolation_lo, const float* isolation_hi,
                          const SagePurityOutput* result, const char* const* filenames, uint32_t n_files) {
    if (!path || !result || (n_files && !filenames) ||
        (n_rows && (!psm_id || !file_id || !spec_ids || !charge || !ms1_ids || !isolation_lo || !isolation_hi || !result->n_window ||
                    !result->n_matched || !result->total || !result->matched || !result->below || !result->purity)))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_purity: null argument");
    for (uint64_t r = 0; r < n_rows; ++r)
        if (file_id[r] >= n_files || !filenames[file_id[r]] || !spec_ids[r])
            return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_purity: file id out of range or null id");
    std::string err;
    if (!write_purity(path, n_rows, psm_id, file_id, spec_ids, charge, ms1_ids, isolation_lo, isolation_hi, *result, filenames, err))
        return fail(SAGE_HIP_ERR_INVALID, err);
    return SAGE_HIP_OK;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int sage_hip_hostdb_build(const char* fasta_text, const SageDbParams* params, SageHostDb** out) {
    if (!fasta_text || !params || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    try {
        auto h = std::make_unique<SageHostDb>();
        h->db = build_database(fasta_text, config_from_params(*params));
        *out = h.release();
        return SAGE_HIP_OK;
    } catch (const std::exception& e) {
        return fail(SAGE_HIP_ERR_INVALID, e.what());
    }
}
int sage_hip_hostdb_build_chunk(const char* fasta_text, const SageDbParams* params, uint64_t first_target, uint64_t n_targets,
                                SageHostDb** out) {
    if (!fasta_text || !params || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    try {
        auto h = std::make_unique<SageHostDb>();
        h->db = build_database(fasta_text, config_from_params(*params), first_target, n_targets);
        *out = h.release();
        return SAGE_HIP_OK;
    } catch (const std::exception& e) {
        return fail(SAGE_HIP_ERR_INVALID, e.what());
    }
}
int sage_hip_fasta_num_targets(const char* fasta_text, const SageDbParams* params, uint64_t* out) {
    if (!fasta_text || !params || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    *out = fasta_num_targets(fasta_text, config_from_params(*params));
    return SAGE_HIP_OK;
}
int sage_hip_prefilter_chunk_size(const char* fasta_text, const SageDbParams* params, uint64_t requested, uint64_t* out) {
    if (!fasta_text || !params || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    *out = prefilter_chunk_size(fasta_text, config_from_params(*params), requested);
    return SAGE_HIP_OK;
}
int sage_hip_hostdb_merge_kept(const SageHostDb* const* chunks, const uint8_t* const* keep, uint32_t n_chunks,
                               const SageDbParams* params, SageHostDb** out) {
    if ((n_chunks && (!chunks || !keep)) || !params || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    try {
        std::vector<const HostDb*> dbs;
        std::vector<const uint8_t*> masks;
        for (uint32_t c = 0; c < n_chunks; ++c) {
            if (!chunks[c] || !keep[c]) return fail(SAGE_HIP_ERR_INVALID, "null chunk");
            dbs.push_back(&chunks[c]->db);
            masks.push_back(keep[c]);
        }
        auto h = std::make_unique<SageHostDb>();
        h->db = merge_kept(dbs, masks, config_from_params(*params));
        *out = h.release();
        return SAGE_HIP_OK;
    } catch (const std::exception& e) {
        return fail(SAGE_HIP_ERR_INVALID, e.what());
    }
}
void sage_hip_hostdb_free(SageHostDb* db) { delete db; }
int sage_hip_hostdb_view(const SageHostDb* db, SageDbView* out) {
    if (!db || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    *out = db->db.view();
    return SAGE_HIP_OK;
}
static uint64_t copy_out(const std::string& s, char* out, uint64_t cap) {
    if (out && cap >= s.size() + 1) std::memcpy(out, s.c_str(), s.size() + 1);
    return s.size() + 1;
}
uint64_t sage_hip_hostdb_peptide_string(const SageHostDb* db, uint64_t i, char* out, uint64_t cap) {
    if (!db || i >= db->db.n_peptides()) return 0;
    return copy_out(db->db.peptide_string(i), out, cap);
}
uint64_t sage_hip_hostdb_peptide_proteins(const SageHostDb* db, uint64_t i, char* out, uint64_t cap) {
    if (!db || i >= db->db.n_peptides()) return 0;
    return copy_out(db->db.peptide_proteins(i), out, cap);
}
int sage_hip_hostdb_peptide_info(const SageHostDb* db, uint64_t i, uint32_t* num_proteins, uint8_t* semi_enzymatic) {
    if (!db || i >= db->db.n_peptides()) return fail(SAGE_HIP_ERR_INVALID, "peptide index out of range");
    if (num_proteins) *num_proteins = (uint32_t)(db->db.pep_protein_off[i + 1] - db->db.pep_protein_off[i]);
    if (semi_enzymatic) *semi_enzymatic = db->db.semi[i];
    return SAGE_HIP_OK;
}
int sage_hip_mzml_read(const char* path, uint32_t file_id, int ms_level, SageMzml** out) {
    return sage_hip_mzml_read_sn(path, file_id, ms_level, -1, out);
}
int sage_hip_mzml_read_sn(const char* path, uint32_t file_id, int ms_level, int sn_level, SageMzml** out) {
    if (!path || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_mzml_read: null argument");
    auto h = std::make_unique<SageMzml>();
    std::string err;
    try {
        if (!read_mzml(path, file_id, ms_level, sn_level, h->run, err)) return fail(SAGE_HIP_ERR_INVALID, err);
    } catch (const std::exception& e) {
        return fail(SAGE_HIP_ERR_INVALID, e.what());
    }
    *out = h.release();
    return SAGE_HIP_OK;
}
// Inputs the reference refuses to SEARCH (it panics while processing them; the reader itself accepts them): profile-mode MS2
// spectra (spectrum.rs:280-286 — Representation defaults to Profile, so a spectrum without the centroid term counts) and MS2
// spectra without a precursor (scoring.rs:466-468).  Call before preprocessing / scoring a run.
int sage_hip_mzml_check_searchable(const SageMzml* run) {
    if (!run) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_mzml_check_searchable: null argument");
    const MzmlRun& r = run->run;
    for (uint64_t i = 0; i < r.n(); ++i) {
        if (r.ms_level[i] < 2) continue;
        const char* id = r.ids.data() + r.id_off[i];
        if (!r.centroid[i]) return fail(SAGE_HIP_ERR_INVALID, std::string("Scan ") + id + " contains profile data! Please convert to centroid");
        if (!r.has_precursor[i]) return fail(SAGE_HIP_ERR_INVALID, std::string("missing MS1 precursor for ") + id);
    }
    return SAGE_HIP_OK;
}
int sage_hip_mzml_view(const SageMzml* run, SageRawBatch* out) {
    if (!run || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_mzml_view: null argument");
    const MzmlRun& r = run->run;
    out->n_spectra = (uint32_t)r.n();
    out->peak_off = r.peak_off.data();
    out->mz = r.mz.data();
    out->intensities = r.intensities.data();
    out->precursor_mz = r.precursor_mz.data();
    out->precursor_charge = r.precursor_charge.data();
    out->isolation_lo = r.isolation_lo.data();
    out->isolation_hi = r.isolation_hi.data();
    out->scan_start_time = r.scan_start_time.data();
    out->inverse_ion_mobility = r.inverse_ion_mobility.data();
    out->file_id = r.file_id.data();
    return SAGE_HIP_OK;
}
const char* sage_hip_mzml_spectrum_id(const SageMzml* run, uint64_t i) {
    if (!run || i >= run->run.n()) return nullptr;
    return run->run.ids.data() + run->run.id_off[i];
}
float sage_hip_mzml_ion_injection_time(const SageMzml* run, uint64_t i) {
    if (!run || i >= run->run.n()) return NAN;
    return run->run.ion_injection_time[i];
}
const char* sage_hip_mzml_precursor_ref(const SageMzml* run, uint64_t i) {
    if (!run || i >= run->run.n()) return nullptr;
    return run->run.precursor_refs.data() + run->run.ref_off[i];
}
const float* sage_hip_mzml_mobility(const SageMzml* run) {
    if (!run || run->run.has_mobility.empty()) return nullptr;
    return run->run.mobility.data();
}
int sage_hip_mzml_has_mobility(const SageMzml* run, uint8_t* out) {
    if (!run || (!out && run->run.n())) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_mzml_has_mobility: null argument");
    const MzmlRun& r = run->run;
    for (uint64_t i = 0; i < r.n(); ++i) out[i] = r.has_mobility.empty() ? 0 : r.has_mobility[i];
    return SAGE_HIP_OK;
}
void sage_hip_mzml_free(SageMzml* run) { delete run; }
int sage_hip_mgf_read(const char* path, uint32_t file_id, SageMzml** out) {
    if (!path || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_mgf_read: null argument");
    auto h = std::make_unique<SageMzml>();
    std::string err;
    try {
        if (!read_mgf(path, file_id, h->run, err)) return fail(SAGE_HIP_ERR_INVALID, err);
    } catch (const std::exception& e) {
        return fail(SAGE_HIP_ERR_INVALID, e.what());
    }
    *out = h.release();
    return SAGE_HIP_OK;
}
int sage_hip_mzml_isolation_kinds(const SageMzml* run, uint8_t* out) {
    if (!run || (!out && run->run.n())) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_mzml_isolation_kinds: null argument");
    const MzmlRun& r = run->run;
    for (uint64_t i = 0; i < r.n(); ++i) out[i] = r.iso_kind.empty() ? (uint8_t)SAGE_TOL_DA : r.iso_kind[i];
    return SAGE_HIP_OK;
}
int sage_hip_mzml_charge_zero(const SageMzml* run, uint8_t* out) {
    if (!run || (!out && run->run.n())) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_mzml_charge_zero: null argument");
    const MzmlRun& r = run->run;
    for (uint64_t i = 0; i < r.n(); ++i) out[i] = r.charge_zero.empty() ? 0 : r.charge_zero[i];
    return SAGE_HIP_OK;
}
int sage_hip_parse_f32(const char* token, uint64_t len, float* out) {
    if ((!token && len) || !out) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_parse_f32: null argument");
    return parse_f32_rust(token, token + len, *out) ? SAGE_HIP_OK : fail(SAGE_HIP_ERR_INVALID, "invalid float literal");
}
int sage_hip_write_results(const char* path, int format, const SageHostDb* db, const SageFeature* features, uint64_t n,
                           const uint64_t* order, const uint64_t* psm_id, const char* const* filenames, uint32_t n_files,
                           const char* const* spec_ids, const SagePostColumns* post) {
    if (!path || !db || (n && (!features || !psm_id || !filenames || !spec_ids)))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_results: null argument");
    if (format != SAGE_FORMAT_TSV && format != SAGE_FORMAT_PIN) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_results: unknown format");
    for (uint64_t r = 0; order && r < n; ++r)
        if (order[r] >= n) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_results: order entry out of range");
    std::string err;
    if (!write_results(path, format, db->db, features, n, order, psm_id, filenames, n_files, spec_ids, post, err))
        return fail(SAGE_HIP_ERR_INVALID, err);
    return SAGE_HIP_OK;
}
int sage_hip_write_results_grouped(const char* path, int format, const SageHostDb* db, const SageFeature* features, uint64_t n,
                                   const uint64_t* order, const uint64_t* psm_id, const char* const* filenames, uint32_t n_files,
                                   const char* const* spec_ids, const SagePostColumns* post, const SageGroupColumns* groups) {
    if (!path || !db || (n && (!features || !psm_id || !filenames || !spec_ids)))
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_results_grouped: null argument");
    if (format != SAGE_FORMAT_TSV && format != SAGE_FORMAT_PIN)
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_results_grouped: unknown format");
    for (uint64_t r = 0; order && r < n; ++r)
        if (order[r] >= n) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_results_grouped: order entry out of range");
    for (uint64_t s = 0; groups && groups->strings && s < groups->n_strings; ++s)
        if (!groups->strings[s]) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_write_results_grouped: null string");
    std::string err;
    if (!write_results_grouped(path, format, db->db, features, n, order, psm_id, filenames, n_files, spec_ids, post, groups, err))
        return fail(SAGE_HIP_ERR_INVALID, err);
    return SAGE_HIP_OK;
}
uint64_t sage_hip_hostdb_protein_name(const SageHostDb* db, uint64_t id, char* out, uint64_t cap) {
    if (!db || id >= db->db.protein_names.size()) return 0;
    return copy_out(db->db.protein_names[id], out, cap);
}
int sage_hip_hostdb_feature_peptides(const SageHostDb* db, const uint32_t* peptide_idx, uint64_t n, uint64_t* seq_off, uint8_t* seq,
                                     float* monoisotopic) {
    if (!db || (n && !peptide_idx) || !seq_off) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_hostdb_feature_peptides: null argument");
    const HostDb& d = db->db;
    uint64_t off = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (peptide_idx[i] >= d.n_peptides()) return fail(SAGE_HIP_ERR_INVALID, "peptide index out of range");
        const uint64_t p = peptide_idx[i], len = d.seq_off[p + 1] - d.seq_off[p];
        seq_off[i] = off;
        if (seq) std::memcpy(seq + off, d.seq.data() + d.seq_off[p], len);
        if (monoisotopic) monoisotopic[i] = d.pep_mono[p];
        off += len;
    }
    seq_off[n] = off;
    return SAGE_HIP_OK;
}
int sage_hip_hostdb_isomer_groups(const SageHostDb* db, uint32_t* group_of, uint64_t* group_off, uint32_t* members, uint64_t* n_groups,
                                  uint64_t* n_members) {
    if (!db || !n_groups || !n_members) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_hostdb_isomer_groups: null argument");
    std::lock_guard<std::mutex> lock(db->iso_mu);
    if (!db->iso_made) {
        db->db.isomer_groups(db->iso_of, db->iso_off, db->iso_members);
        db->iso_made = true;
    }
    const std::vector<uint32_t>&of = db->iso_of, &mem = db->iso_members;
    const std::vector<uint64_t>& off = db->iso_off;
    const bool sizing = !group_off && !members;
    if (!sizing) {
        if (!group_off || (!members && !mem.empty())) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_hostdb_isomer_groups: group_off and members go together");
        std::memcpy(group_off, off.data(), off.size() * sizeof(uint64_t));
        if (!mem.empty()) std::memcpy(members, mem.data(), mem.size() * sizeof(uint32_t));
    }
    if (group_of && !of.empty()) std::memcpy(group_of, of.data(), of.size() * sizeof(uint32_t));
    *n_groups = off.size() - 1;
    *n_members = mem.size();
    return SAGE_HIP_OK;
}
int sage_hip_hostdb_competition_keys(const SageHostDb* db, const uint32_t* peptide_idx, uint64_t n, uint32_t* peptide_key,
                                     uint32_t* n_peptide_keys, uint32_t* protein_key, uint32_t* n_protein_keys) {
    if (!db || (n && (!peptide_idx || !peptide_key || !protein_key)) || !n_peptide_keys || !n_protein_keys)
        return fail(SAGE_HIP_ERR_INVALID, "sage_hip_hostdb_competition_keys: null argument");
    for (uint64_t i = 0; i < n; ++i)
        if (peptide_idx[i] >= db->db.n_peptides()) return fail(SAGE_HIP_ERR_INVALID, "peptide index out of range");
    db->db.competition_keys(peptide_idx, n, peptide_key, *n_peptide_keys, protein_key, *n_protein_keys);
    return SAGE_HIP_OK;
}
uint64_t sage_hip_process_ms2(uint64_t take_top_n, int deisotope, float min_deisotope_mz, const float* mz,
                              const float* intensity, uint64_t n, uint8_t precursor_charge, float* out_mass,
                              float* out_intensity, float* out_tic) {
    return process_ms2(take_top_n, deisotope != 0, min_deisotope_mz, mz, intensity, n, precursor_charge, out_mass,
                       out_intensity, out_tic);
}

}  // extern "C"
