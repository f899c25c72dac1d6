// capi_db.hip — the device database of the C ABI (include/sage_hip.h): sage_hip_db_create and what reads a SageDeviceDb back.
// Host code only (the kernels of the index build: index_build.hip).
#include "capi_state.h"

// where each tile of 2^shift consecutive peptides starts in the peptide-major fragment list
static std::vector<uint64_t> tile_offsets(const std::vector<uint64_t>& pm_off, uint64_t np, uint64_t n_tiles, uint32_t shift) {
    std::vector<uint64_t> tile_off(n_tiles + 1, 0);
    for (uint64_t t = 0; t < n_tiles; t++) tile_off[t + 1] = pm_off[std::min<uint64_t>(np, (t + 1) << shift)];
    return tile_off;
}

extern "C" {

int sage_hip_db_create(const SageDbView* v, int device, SageDeviceDb** out) {
    if (!v || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    if (v->n_peptides >= 0xFFFFFFFFull) return fail(SAGE_HIP_ERR_UNSUPPORTED, "more than 2^32-2 peptides");
    if (v->n_ion_kinds > 8) return fail(SAGE_HIP_ERR_INVALID, "more than 8 ion kinds");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SAGE_HIP_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(SAGE_HIP_ERR_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    auto d = std::make_unique<SageDeviceDb>();
    d->device = device;
    const uint64_t np = v->n_peptides;
    const uint32_t nk = v->n_ion_kinds;

    // complete ion table for rescoring (IonSeries for every configured kind, ion_series.rs:36-85)
    std::vector<uint64_t> ion_off(np + 1, 0);
    std::vector<uint32_t> info(np);
    uint32_t max_ions = 0, max_len = 0;
    d->h_len.reserve(np);
    for (uint64_t i = 0; i < np; i++) {
        const uint64_t len = v->seq_off[i + 1] - v->seq_off[i];
        // (the production rescoring kernel keeps a candidate's longest-run state in 10-bit fields — kernels.hip, run_matched_packed —;
        // a database with longer peptides is scored by the general instances: scorer_init, DevScorer::long_runs)
        if (len > 65535) return fail(SAGE_HIP_ERR_UNSUPPORTED, "peptide longer than 65535 residues");  // (pep_info: 16 bits)
        max_len = std::max<uint32_t>(max_len, (uint32_t)len);
        d->h_len.push_back((uint16_t)len);
        const uint64_t cnt = (len ? len - 1 : 0) * nk;
        ion_off[i + 1] = ion_off[i] + cnt;
        max_ions = std::max<uint32_t>(max_ions, (uint32_t)cnt);
        info[i] = (uint32_t)len | ((uint32_t)(v->decoy[i] ? 1 : 0) << 16) | ((uint32_t)v->missed_cleavages[i] << 24);
    }
    uint32_t tile_shift = TILE_SHIFT_MAX;
    if (const char* e = getenv("SAGE_HIP_TILE_SHIFT")) tile_shift = (uint32_t)std::min((int)TILE_SHIFT_MAX, std::max(11, atoi(e)));
    const uint64_t n_tiles = std::max<uint64_t>(1, (np + (1ull << tile_shift) - 1) >> tile_shift);
    // 1/256 Da cells.  The scale is a power of two, so `m/z * scale` is exact in f32 and a fragment-tolerance window
    // [lo, hi] maps to the cell range [floor(lo*scale), floor(hi*scale)] with no safety margin.
    const float lut_scale = 256.0f;
    uint32_t lut_stride = 0;
    uint64_t nf = v->n_fragments;
    d->h_pep_mono.assign(v->pep_mono, v->pep_mono + np);
    std::vector<uint64_t> pm_off(np + 1, 0);  // fragment offset of every peptide
    if (!v->fragments) {
        for (uint64_t i = 0; i < np; i++) {
            const uint64_t len = v->seq_off[i + 1] - v->seq_off[i], lm1 = len ? len - 1 : 0;
            pm_off[i + 1] = pm_off[i] + (lm1 > v->min_ion_index ? lm1 - v->min_ion_index : 0) * nk;  // database.rs:281-292
        }
        nf = pm_off[np];
    } else {
        // group IndexedDatabase.fragments by peptide (counting sort): tiles are runs of 2^tile_shift consecutive peptides
        for (uint64_t i = 0; i < nf; i++) {
            if (v->fragments[i].peptide_index >= np) return fail(SAGE_HIP_ERR_INVALID, "fragment peptide_index out of range");
            pm_off[v->fragments[i].peptide_index + 1]++;
        }
        for (uint64_t i = 0; i < np; i++) pm_off[i + 1] += pm_off[i];
    }
    if (nf >= 0xFFFFFFF0ull) return fail(SAGE_HIP_ERR_UNSUPPORTED, "more than 2^32-16 fragments");
    const std::vector<uint64_t> tile_off = tile_offsets(pm_off, np, n_tiles, tile_shift);
    auto upload_peptide_tables = [&]() -> int {  // (each build at its own point: the order of the device build's allocations stays)
        HIP_TRY(d->pep_mono.upload(v->pep_mono, np));
        HIP_TRY(d->ion_off.upload(ion_off.data(), np + 1));
        HIP_TRY(d->pm_off.upload(pm_off.data(), np + 1));
        return SAGE_HIP_OK;
    };
    if (!v->fragments) {
        // ---- Parameters::build_from_peptides (database.rs:265-346) on the device: index_build.hip ----
        const uint64_t total_res = np ? v->seq_off[np] : 0;
        DevBuf<uint64_t> d_seq_off, d_tile_off;
        DevBuf<uint8_t> d_seq, d_kinds;
        DevBuf<float> d_mods, d_nterm;
        HIP_TRY(d_seq_off.upload(v->seq_off, np + 1));
        HIP_TRY(d_seq.upload(v->seq, total_res));
        HIP_TRY(d_mods.upload(v->mods, total_res));
        HIP_TRY(d_nterm.upload(v->nterm, np));
        HIP_TRY(d_kinds.upload(v->ion_kinds, nk));
        HIP_TRY(d_tile_off.upload(tile_off.data(), n_tiles + 1));
        if (const int rc = upload_peptide_tables()) return rc;
        HIP_TRY(d->ions.alloc(ion_off[np] + 8));  // (padded: the rescoring kernel reads ions four at a time)
        HIP_TRY(d->pm_frag.alloc(nf));
        HIP_TRY(d->tm_frag.alloc(nf + 2));
        hipError_t be = (hipError_t)generate_fragments_on_device(np, nk, d_kinds.p, d_seq_off.p, d_seq.p, d_mods.p, d_nterm.p, d->pep_mono.p,
                                                                v->min_ion_index, d->ion_off.p, d->pm_off.p, d->ions.p, d->pm_frag.p, nullptr);
        if (be == hipSuccess)
            be = (hipError_t)build_tile_copy_on_device(d->pm_frag.p, nf, tile_shift, (uint32_t)n_tiles, d_tile_off.p, lut_scale,
                                                       d->tm_frag.p, d->tm_lut, &lut_stride, nullptr);
        if (be != hipSuccess) return fail(status_of(be), std::string("device index build: ") + hipGetErrorString(be));
        // (here, not behind the branches: the build's inputs above are released after this allocation, as they always were — the
        // sequence of allocations and releases of the device build decides where a large index lies in HBM and its peak)
        HIP_TRY(d->pep_info.upload(info.data(), np));
    } else {
        std::vector<SageTheoretical> tm(nf + 2, SageTheoretical{0xFFFFFFFFu, 0.0f});
        {
            std::vector<uint64_t> cur(pm_off.begin(), pm_off.end() - 1);
            for (uint64_t i = 0; i < nf; i++) tm[cur[v->fragments[i].peptide_index]++] = v->fragments[i];
        }
        HIP_TRY(d->pm_frag.upload(tm.data(), nf));  // (before the tiles are re-sorted by m/z below)
        if (const int rc = upload_peptide_tables()) return rc;
        std::vector<float> ions(ion_off[np] + 8);  // (padded: the rescoring kernel reads ions four at a time)
        parallel_for(np, 4096, [&](size_t ib, size_t ie, unsigned) {
            for (size_t i = ib; i < ie; i++) {
                const uint64_t len = v->seq_off[i + 1] - v->seq_off[i];
                const uint64_t lm1 = len ? len - 1 : 0;
                for (uint32_t k = 0; k < nk; k++)
                    ion_series_flat(v->seq + v->seq_off[i], v->mods + v->seq_off[i], len, v->nterm[i], v->pep_mono[i],
                                    v->ion_kinds[k], ions.data() + ion_off[i] + (uint64_t)k * lm1);
            }
        });
        // tile-major copy for large precursor windows: tile = peptide_index >> tile_shift, (m/z, peptide) order inside a
        // tile, and a per-tile position table tm_lut[t][c] = first position of tile t with m/z >= c / lut_scale.
        parallel_for(n_tiles, 1, [&](size_t tb, size_t te, unsigned) {
            for (size_t t = tb; t < te; t++)
                std::sort(tm.begin() + tile_off[t], tm.begin() + tile_off[t + 1], [](const SageTheoretical& x, const SageTheoretical& y) {
                    const int32_t kx = sagecore::order_key(x.fragment_mz), ky = sagecore::order_key(y.fragment_mz);
                    return kx != ky ? kx < ky : x.peptide_index < y.peptide_index;
                });
        });
        float max_mz = 0.0f;
        for (uint64_t i = 0; i < nf; i++)
            if (tm[i].fragment_mz > max_mz && std::isfinite(tm[i].fragment_mz)) max_mz = tm[i].fragment_mz;
        lut_stride = (uint32_t)std::min<double>(std::ceil((double)max_mz * lut_scale) + 3.0, 64.0e6);
        if ((double)n_tiles * lut_stride > 4.0e9) return fail(SAGE_HIP_ERR_UNSUPPORTED, "tile position table larger than 16 GB");
        std::vector<uint32_t> lut((size_t)n_tiles * lut_stride, (uint32_t)tile_off[n_tiles]);
        parallel_for(n_tiles, 1, [&](size_t tb, size_t te, unsigned) {
            for (size_t t = tb; t < te; t++) {
                uint64_t pos = tile_off[t];
                const uint64_t tend = tile_off[t + 1];
                auto cell = [&](uint32_t c) -> uint32_t& { return lut[tm_lut_index((uint32_t)t, c, lut_stride)]; };
                for (uint32_t c = 0; c < lut_stride; c++) {
                    const double edge = (double)c / (double)lut_scale;
                    // NaN and m/z beyond the table (non-finite or > 250 kDa) compare false and stay in the last cell's run
                    while (pos < tend && (double)tm[pos].fragment_mz < edge) pos++;
                    cell(c) = (uint32_t)pos;
                }
                cell(0) = (uint32_t)tile_off[t];  // a window starting below cell 0 starts at the tile's first entry
                cell(lut_stride - 1) = (uint32_t)tend;
            }
        });
        HIP_TRY(d->tm_frag.upload(tm.data(), tm.size()));
        HIP_TRY(d->tm_lut.upload(lut.data(), lut.size()));
        HIP_TRY(d->ions.upload(ions.data(), ions.size()));
        HIP_TRY(d->pep_info.upload(info.data(), np));
    }
    {
        // small-tile copy for the narrow kernel (device_types.h: tm2_*), sorted on the device from the peptide-major list
        // 2^11 peptides per small tile (round 4; 2^12 before): a +-10 ppm window of a human digest holds ~200 candidates, so of a
        // tile's run for one fragment window only candidates / tile-size are inside the precursor window — the rest is fetched and
        // thrown away, and prelim_kernel follows its line traffic.  C3, prelim ms per 500 000 spectra by shift 13 / 12 / 11 / 10 / 9 / 8:
        // 2.26 / 1.86 / 1.68 / 1.67 / 1.83 / 2.20 (smaller tiles: more table rows, each reused by fewer spectra; 62 500-spectrum
        // steps favour 11 over 10).  The table doubles to 1.5 GB for C3.
        uint32_t tile2_shift = 11;
        if (const char* e = getenv("SAGE_HIP_TILE2_SHIFT")) tile2_shift = (uint32_t)std::min(16, std::max(6, atoi(e)));
        float lut2_scale = 32.0f;  // cells per Da (a power of two, like lut_scale)
        if (const char* e = getenv("SAGE_HIP_LUT2_SCALE")) {  // (experiments: 8 .. 256, rounded down to a power of two)
            const int v = std::min(256, std::max(8, atoi(e)));
            lut2_scale = (float)(1 << (31 - __builtin_clz((unsigned)v)));
        }
        const uint64_t n_tiles2 = std::max<uint64_t>(1, (np + (1ull << tile2_shift) - 1) >> tile2_shift);
        const std::vector<uint64_t> tile2_off = tile_offsets(pm_off, np, n_tiles2, tile2_shift);
        DevBuf<uint64_t> d_tile2_off;
        HIP_TRY(d_tile2_off.upload(tile2_off.data(), n_tiles2 + 1));
        HIP_TRY(d->tm2_frag.alloc(nf + 2));
        DevBuf<uint32_t> lut2;  // the row-major table
        uint32_t lut2_stride = 0;
        const hipError_t be = (hipError_t)build_tile_copy_on_device(d->pm_frag.p, nf, tile2_shift, (uint32_t)n_tiles2, d_tile2_off.p,
                                                                    lut2_scale, d->tm2_frag.p, lut2, &lut2_stride, nullptr);
        if (be != hipSuccess) return fail(status_of(be), std::string("device index build: ") + hipGetErrorString(be));
        // the table in succinct form (index_build.hip: build_succinct_lut_on_device; the row-major table is its input only —
        // 1.5 GB for C3 that the narrow kernel no longer reads a line of per lookup)
        uint32_t lut2_words = 0;
        const hipError_t se = (hipError_t)build_succinct_lut_on_device(lut2.p, (uint32_t)n_tiles2, lut2_stride, d->tm2_l1, d->tm2_pos, &lut2_words, nullptr);
        lut2.release();
        if (se != hipSuccess) return fail(status_of(se), std::string("device index build (succinct table): ") + hipGetErrorString(se));
        d->view.tm2_frag = d->tm2_frag.p;
        d->view.tm2_l1 = d->tm2_l1.p;
        d->view.tm2_pos = d->tm2_pos.p;
        d->view.lut2_words = lut2_words;
        d->view.tile2_shift = tile2_shift;
        d->view.n_tiles2 = (uint32_t)n_tiles2;
        d->view.lut2_stride = lut2_stride;
        d->view.lut2_scale = lut2_scale;
    }
    d->max_ions = max_ions;
    d->max_len = max_len;
    HIP_TRY((hipError_t)ion_abs_range_on_device(d->ions.p, ion_off[np], &d->ion_lo_bits, &d->ion_hi_bits));
    {  // the position table of the precursor-window search key
        uint32_t bins = 0;
        float inv_w = 0.0f;
        // (SAGE_HIP_NO_PEP_LUT=1: without — every window through the full search; tests hold the two against each other)
        const bool off = getenv("SAGE_HIP_NO_PEP_LUT") && getenv("SAGE_HIP_NO_PEP_LUT")[0] == '1';
        const hipError_t be = off ? hipSuccess
                                  : (hipError_t)build_peptide_mass_lut(d->pep_mono.p, (uint32_t)np, np ? d->h_pep_mono[np - 1] : 0.0f, d->pep_lut, &bins, &inv_w, nullptr);
        if (be != hipSuccess) return fail(status_of(be), std::string("peptide-mass table: ") + hipGetErrorString(be));
        d->view.pep_lut = d->pep_lut.p;
        d->view.pep_lut_bins = bins;
        d->view.pep_lut_inv_w = inv_w;
    }
    d->view.pep_mono = d->pep_mono.p;
    d->view.np = (uint32_t)np;
    d->view.pm_frag = d->pm_frag.p;
    d->view.pm_off = d->pm_off.p;
    d->view.ions = d->ions.p;
    d->view.ion_off = d->ion_off.p;
    d->view.pep_info = d->pep_info.p;
    d->view.tm_frag = d->tm_frag.p;
    d->view.tm_lut = d->tm_lut.p;
    d->view.tile_shift = tile_shift;
    d->view.n_tiles = (uint32_t)n_tiles;
    d->view.lut_stride = lut_stride;
    d->view.lut_scale = lut_scale;
    d->view.nf = nf;
    std::memset(d->view.ion_kinds, 0, sizeof d->view.ion_kinds);
    for (uint32_t k = 0; k < nk; k++) d->view.ion_kinds[k] = v->ion_kinds[k];
    d->view.n_kinds = nk;
    if (!getenv("SAGE_HIP_KEEP_PM_FRAG")) {
        d->pm_frag.release();
        d->view.pm_frag = nullptr;
    }
    d->bytes = d->pep_mono.bytes() + d->pep_lut.bytes() + d->pm_frag.bytes() + d->pm_off.bytes() + d->ions.bytes() + d->ion_off.bytes() +
               d->pep_info.bytes() + d->tm_frag.bytes() + d->tm_lut.bytes() + d->tm2_frag.bytes() + d->tm2_l1.bytes() + d->tm2_pos.bytes();
    *out = d.release();
    return SAGE_HIP_OK;
}

}  // extern "C"

// the peptide-major fragment list for a batch that takes the stream variant of the preliminary kernels (SageDeviceDb::pm_frag)
int ensure_pm_frag(SageDeviceDb* db) {
    std::lock_guard<std::mutex> lock(db->pm_mu);
    if (db->view.pm_frag) return SAGE_HIP_OK;
    HIP_TRY(db->pm_frag.alloc((size_t)db->view.nf + 2));
    const hipError_t be = (hipError_t)rebuild_peptide_major_on_device(db->tm_frag.p, db->view.nf, db->pm_frag.p, nullptr);
    if (be != hipSuccess) {
        db->pm_frag.release();
        return fail(status_of(be), std::string("peptide-major fragment list: ") + hipGetErrorString(be));
    }
    db->bytes += db->pm_frag.bytes();
    db->view.pm_frag = db->pm_frag.p;
    return SAGE_HIP_OK;
}

extern "C" {

void sage_hip_db_destroy(SageDeviceDb* db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    delete db;
}
uint64_t sage_hip_db_device_bytes(const SageDeviceDb* db) { return db ? db->bytes : 0; }

// debugging aid: the scalars of the device database's layout (what DevDbView and SageDeviceDb hold beside the table pointers)
int sage_hip_debug_db_layout(SageDeviceDb* db, SageDbLayout* out) {
    if (!db || !out) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    const DevDbView& v = db->view;
    std::memset(out, 0, sizeof *out);
    out->np = v.np;
    out->nf = v.nf;
    out->tile_shift = v.tile_shift;
    out->n_tiles = v.n_tiles;
    out->lut_stride = v.lut_stride;
    out->lut_scale = v.lut_scale;
    out->tile2_shift = v.tile2_shift;
    out->n_tiles2 = v.n_tiles2;
    out->lut2_stride = v.lut2_stride;
    out->lut2_scale = v.lut2_scale;
    out->lut2_words = v.lut2_words;
    out->pep_lut_bins = v.pep_lut_bins;
    out->pep_lut_inv_w = v.pep_lut_inv_w;
    out->ion_lo_bits = db->ion_lo_bits;
    out->ion_hi_bits = db->ion_hi_bits;
    out->max_ions = db->max_ions;
    out->max_len = db->max_len;
    out->tm2_pos_len = db->tm2_pos.n;
    return SAGE_HIP_OK;
}

// debugging aid: one table of the device database, as it lies in HBM (include/sage_hip.h: SAGE_DB_*)
int sage_hip_debug_db_table(SageDeviceDb* db, int table, void* out, uint64_t cap_bytes, uint64_t* out_bytes) {
    if (!db || !out_bytes) return fail(SAGE_HIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(db->device));
    if (table == SAGE_DB_PM_FRAG)
        if (int rc = ensure_pm_frag(db)) return rc;
    const void* src = nullptr;
    uint64_t bytes = 0;
    switch (table) {
        case SAGE_DB_IONS: src = db->ions.p; bytes = db->ions.bytes() - 8 * sizeof(float); break;  // (padded: sage_hip_db_create)
        case SAGE_DB_ION_OFF: src = db->ion_off.p; bytes = db->ion_off.bytes(); break;
        case SAGE_DB_PM_OFF: src = db->pm_off.p; bytes = db->pm_off.bytes(); break;
        case SAGE_DB_PEP_INFO: src = db->pep_info.p; bytes = db->pep_info.bytes(); break;
        case SAGE_DB_PEP_MONO: src = db->pep_mono.p; bytes = db->pep_mono.bytes(); break;
        case SAGE_DB_PEP_LUT: src = db->pep_lut.p; bytes = db->pep_lut.bytes(); break;  // (never allocated: no table)
        case SAGE_DB_PM_FRAG: src = db->pm_frag.p; bytes = db->pm_frag.bytes(); break;
        case SAGE_DB_TM_FRAG: src = db->tm_frag.p; bytes = db->tm_frag.bytes(); break;
        case SAGE_DB_TM2_FRAG: src = db->tm2_frag.p; bytes = db->tm2_frag.bytes(); break;
        case SAGE_DB_TM_LUT: src = db->tm_lut.p; bytes = db->tm_lut.bytes(); break;
        case SAGE_DB_TM2_L1: src = db->tm2_l1.p; bytes = db->tm2_l1.bytes(); break;
        case SAGE_DB_TM2_POS: src = db->tm2_pos.p; bytes = db->tm2_pos.bytes(); break;
        default: return fail(SAGE_HIP_ERR_INVALID, "sage_hip_debug_db_table: unknown table id");
    }
    *out_bytes = bytes;
    if (!out || !bytes) return SAGE_HIP_OK;
    if (cap_bytes < bytes) return fail(SAGE_HIP_ERR_INVALID, "sage_hip_debug_db_table: buffer smaller than the table");
    HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return SAGE_HIP_OK;
}

}  // extern "C"
