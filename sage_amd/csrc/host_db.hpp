// Host-side IndexedDatabase construction for libsage_hip (product code).
// Mirrors sage-core's Parameters::build (crates/sage/src/database.rs:260-364) and everything it
// calls: fasta.rs, enzyme.rs, peptide.rs, modification.rs, ion_series.rs.  Output is the flat
// SoA/AoS layout that include/sage_hip.h's SageDbView exposes and that the device uploader consumes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/sage_hip.h"

namespace sagehip {

// modification.rs:10-17 (ModificationSpecificity); residue < 0 == None
struct ModTarget {
    enum Where : uint8_t { PeptideN, PeptideC, ProteinN, ProteinC, Residue } where;
    int residue;
};
bool parse_mod_target(const char* key, ModTarget& out);  // modification.rs:66-104

struct DbBuildConfig {  // database.rs:122-139 after Builder::make_parameters (:96-115)
    uint64_t bucket_size = 8192;
    uint8_t missed_cleavages = 0;
    size_t min_len = 5, max_len = 50;
    std::string cleave_at = "KR", restrict_ = "P";
    bool c_terminal = true, semi_enzymatic = false;
    float peptide_min_mass = 500.0f, peptide_max_mass = 5000.0f;
    std::vector<uint8_t> ion_kinds = {SAGE_ION_B, SAGE_ION_Y};
    size_t min_ion_index = 2;
    std::vector<std::pair<ModTarget, float>> static_mods;
    std::vector<std::pair<ModTarget, float>> variable_mods;  // flattened (target, mass) pairs
    size_t max_variable_mods = 2;
    std::string decoy_tag = "rev_";
    bool generate_decoys = true;
    bool peptides_only = false;  // stop after reorder_peptides: the device generates the fragment index
};
DbBuildConfig config_from_params(const SageDbParams& p);

struct HostDb {
    std::vector<SageTheoretical> fragments;
    std::vector<float> min_value;
    uint64_t bucket_size = 8192;
    std::vector<float> pep_mono;
    std::vector<uint64_t> seq_off;
    std::vector<uint8_t> seq;
    std::vector<float> mods;
    std::vector<float> nterm, cterm;
    std::vector<uint8_t> decoy, missed, semi, position;  // position: enzyme.rs:64-71 (Nterm, Cterm, Full, Internal)
    std::vector<uint8_t> ion_kinds;
    // protein bookkeeping (not used by the scoring path; kept so writers can be added later)
    std::vector<std::string> protein_names;
    std::vector<uint64_t> pep_protein_off;
    std::vector<uint32_t> pep_protein_ids;
    std::string decoy_tag;
    bool generate_decoys = true;
    uint64_t min_ion_index = 2;

    uint64_t n_peptides() const { return pep_mono.size(); }
    SageDbView view() const;
    std::string peptide_string(uint64_t i) const;
    std::string peptide_proteins(uint64_t i) const;
    void competition_keys(const uint32_t* peptide_idx, uint64_t n, uint32_t* peptide_key, uint32_t& n_peptide_keys,
                          uint32_t* protein_key, uint32_t& n_protein_keys) const;
    // positional isomers: group_of[n_peptides] (0xFFFFFFFF: none), group_off[n_groups + 1] into members
    void isomer_groups(std::vector<uint32_t>& group_of, std::vector<uint64_t>& group_off, std::vector<uint32_t>& members) const;
};

unsigned host_threads();
void parallel_for(size_t n, size_t grain, const std::function<void(size_t, size_t, unsigned)>& f);

HostDb build_database(const std::string& fasta_text, const DbBuildConfig& cfg, uint64_t first_target = 0,
                      uint64_t n_targets = ~0ull);
// the `prefilter` flow of sage-cli (runner.rs:104-127, :143-238)
uint64_t fasta_num_targets(const std::string& fasta_text, const DbBuildConfig& cfg);
uint64_t prefilter_chunk_size(const std::string& fasta_text, const DbBuildConfig& cfg, uint64_t requested);
HostDb merge_kept(const std::vector<const HostDb*>& chunks, const std::vector<const uint8_t*>& keep, const DbBuildConfig& cfg);

// mzml_reader.cpp: the MSn spectra of one mzML file as flat arrays (the layout of SageRawBatch) + their ids
struct MzmlRun {
    std::vector<uint64_t> peak_off;  // [n + 1]
    std::vector<float> mz, intensities;
    std::vector<float> precursor_mz, isolation_lo, isolation_hi, scan_start_time, inverse_ion_mobility;  // NaN == None
    std::vector<uint8_t> precursor_charge;                                                                 // 0 == None
    std::vector<uint8_t> centroid, has_precursor, ms_level;  // Representation::Centroid seen; a <precursor> with a selected ion; level
    std::vector<uint32_t> file_id;
    std::string ids;                 // NUL-separated spectrum ids
    std::vector<uint64_t> id_off;    // [n + 1] into ids
    std::vector<float> ion_injection_time;  // MS:1000927, 0 when absent
    std::string precursor_refs;      // NUL-separated spectrumRef of each kept precursor ("" when absent)
    std::vector<uint64_t> ref_off{0};  // [n + 1] into precursor_refs
    std::vector<uint8_t> iso_kind;     // SAGE_TOL_* of isolation_lo / hi; empty == all SAGE_TOL_DA (mzML)
    std::vector<uint8_t> charge_zero;  // precursors[0].charge == Some(0) (MGF `CHARGE=0`); empty == none
    std::vector<float> mobility;       // per peak, like mz: the ion-mobility array of MS1 spectra; empty == no spectrum has one
    std::vector<uint8_t> has_mobility; // [n] RawSpectrum.mobility is Some; empty == none
    uint64_t n() const { return precursor_mz.size(); }
};
bool read_mzml(const char* path, uint32_t file_id, int ms_level, int sn_level, MzmlRun& run, std::string& err);
bool load_text(const char* path, std::string& text, std::string& err);
// mgf_reader.cpp: sage-cloudpath mgf.rs MgfReader::with_file_id(file_id).parse(..)
bool read_mgf(const char* path, uint32_t file_id, MzmlRun& run, std::string& err);
// str::parse::<f32>() (Rust core dec2flt): grammar and correctly rounded value; false when the token is rejected
bool parse_f32_rust(const char* b, const char* e, float& out);

// writers.cpp
bool write_results(const char* path, int format, const HostDb& db, const SageFeature* f, uint64_t n, const uint64_t* order,
                   const uint64_t* psm_id, const char* const* filenames, uint32_t n_files, const char* const* spec_ids,
                   const SagePostColumns* post, std::string& err);
bool write_lfq(const char* path, const HostDb& db, const SageLfqOutput& g, const uint64_t* rows, uint64_t n_rows,
               const char* const* filenames, uint32_t n_files, std::string& err);
bool write_tmt(const char* path, const char* const* headers, uint32_t n_labels, uint64_t n_rows, const uint32_t* file_id,
               const char* const* spec_ids, const float* ion_injection_time, const float* intensity, const char* const* filenames,
               uint32_t n_files, std::string& err);
bool write_protein_lfq(const char* path, const char* const* protein_names, const uint32_t* rows, uint32_t n_out,
                       const SageProteinLfqOutput& result, const char* const* filenames, uint32_t n_files, std::string& err);
bool write_tmt_rollup(const char* path, const char* first_header, const char* const* headers, uint32_t n_labels, uint64_t n_out,
                      const char* const* names, const uint32_t* plex, const uint32_t* n_psms, const uint32_t* n_peptides,
                      const double* abundance, std::string& err);
bool write_purity(const char* path, uint64_t n_rows, const uint64_t* psm_id, const uint32_t* file_id, const char* const* spec_ids,
                  const uint8_t* charge, const char* const* ms1_ids, const float* isolation_lo, const float* isolation_hi,
                  const SagePurityOutput& result, const char* const* filenames, std::string& err);

// groups.cpp: the host half of protein grouping (protein_grouping.rs:159-231 ProteinGrouper::build)
struct GroupGraph {
    std::vector<uint32_t> protein_name;   // [ProteinIx] dense id of the protein's name (NameIndex), in numbering order
    std::vector<uint8_t> protein_decoy;   // [ProteinIx]
    std::vector<uint32_t> protein_db_id;  // [ProteinIx] a HostDb protein id that carries the name
    uint32_t n_meta = 0;                  // distinct meta-peptides
    std::vector<uint64_t> group_off;      // [groups + 1] into group_proteins (ascending ProteinIx inside a group)
    std::vector<uint32_t> group_proteins;
    std::vector<uint64_t> evidence_off;   // [groups + 1] into evidence: the group's ascending meta-peptide indices
    std::vector<uint32_t> evidence;
    std::vector<uint32_t> edge_group, edge_meta;  // one edge per evidence entry, in group order
    uint32_t n_groups() const { return group_off.empty() ? 0u : (uint32_t)(group_off.size() - 1); }
};
struct NameIndex {  // HostDb protein id -> dense id of its name (two FASTA entries with one accession are one protein)
    std::vector<uint32_t> of_protein;
    uint32_t n_names = 0;
    explicit NameIndex(const HostDb& db);
};
// peptides: ascending, distinct (the selected set P of one pass)
void build_group_graph(const HostDb& db, const NameIndex& names, const uint32_t* peptides, uint64_t n, GroupGraph& out);
// ProteinGroup::format: the group's names (decoy tag where decoy && generate_decoys), sorted, joined by '/'
std::string group_string(const HostDb& db, const GroupGraph& g, uint32_t group);
// protein_groups.hip: sage_hip_protein_groups on the device; `strings` receives the distinct protein_groups strings
int protein_groups_on_device(int device, const HostDb& db, const SageGroupInput& in, SageGroupOutput& out, std::vector<std::string>& strings,
                             std::string& err);
bool write_results_grouped(const char* path, int format, const HostDb& db, const SageFeature* f, uint64_t n, const uint64_t* order,
                           const uint64_t* psm_id, const char* const* filenames, uint32_t n_files, const char* const* spec_ids,
                           const SagePostColumns* post, const SageGroupColumns* groups, std::string& err);

// f32 residue masses, mass.rs:64-76
float residue_mass(uint8_t aa);
// IonSeries (ion_series.rs:36-85) for a flat peptide record; writes L-1 masses to out
void ion_series_flat(const uint8_t* seq, const float* mods, size_t len, float nterm /*NaN none*/, float mono,
                     uint8_t kind, float* out);

// SpectrumProcessor::process for one MS2 spectrum (spectrum.rs:279-412)
uint64_t process_ms2(uint64_t take_top_n, bool deisotope, float min_deisotope_mz, const float* mz,
                     const float* intensity, uint64_t n, uint8_t precursor_charge, float* out_mass,
                     float* out_intensity, float* out_tic);

}  // namespace sagehip
