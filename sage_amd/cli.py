"""JSON-config command line for the search-and-score path — the drop-in for `sage config.json [mzML ...]`.

    python -m sage_amd.cli config.json [-o OUTPUT_DIRECTORY] [-f FASTA] [--annotate-matches] [mzml ...]

Mirrors sage-cli for this path and nothing else: the JSON schema and defaults of
crates/sage-cli/src/input.rs (Input -> Search, :298-385; `database` = sage-core Builder, database.rs:59-139), the per-file
flow of runner.rs (read mzML -> SpectrumProcessor::process -> keep MS2 with >= min_peaks peaks -> Scorer::score,
:311-325, :398-461) and the `results.sage.tsv` / `matched_fragments.sage.tsv` writers (:687-935).  Everything downstream
of Scorer::score is limited to the LDA rescoring, q-values and picked peptide / protein FDR (runner.rs:536-541, on the
device: rescore.hip), label-free MS1 quantification when `quant.lfq` is true (runner.rs:562-575, lfq.hip: `lfq.tsv`) and its
MaxLFQ roll-up to proteins when `quant.protein_lfq` is true too (an addition, protein_lfq.hip: `protein_lfq.tsv`),
isobaric-tag (TMT) reporter-ion quantification when `quant.tmt` is set (runner.rs:334-359, 398-410, tmt.hip: `tmt.tsv`),
its roll-up to proteins when `quant.tmt_rollup` is true too (an addition, tmt_rollup.hip: `tmt_proteins.tsv`),
IDPicker protein groups with the picked protein-group FDR when the configuration names `protein_grouping` or
`protein_grouping_peptide_fdr` (runner.rs:539-549, protein_groups.hip + groups.cpp; see run()) and the optional percolator .pin file;
parquet and cloud IO are out of scope.  The search itself runs on the GPU through libsage_hip.so; there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

from . import output
from ._lib import FEATURE_DTYPE as L_FEATURE_DTYPE
from .api import (LFQ_INTEGRATION, LFQ_SCORING, DatabaseParameters, DeviceDatabase, Isobaric, LfqSettings, RawBatch, Scorer,
                  ScorerParams, SpectrumBatch, SpectrumProcessor, TmtSettings, Tolerance, device_count, lfq, peptide_compositions,
                  NO_MS1, assign_ms1, precursor_purity, predict_rt, protein_groups, protein_lfq, rescore, tmt, tmt_rollup)
from .mgf import TOL_DA, is_mgf, read_mgf_native, read_spectra


def search_parameters(cfg: dict) -> dict:
    """Input::build (input.rs:298-385): defaults of every key the path reads."""
    pc = cfg.get("precursor_charge") or [2, 4]
    if pc[0] > pc[1]:
        raise SystemExit(f"Precursor charges should be specified [low, high], user provided: [{pc[0]}, {pc[1]}]")
    iso = cfg.get("isotope_errors") or [0, 0]
    return dict(
        precursor_tol=Tolerance.from_json(cfg["precursor_tol"]), fragment_tol=Tolerance.from_json(cfg["fragment_tol"]),
        report_psms=cfg.get("report_psms") or 1, max_peaks=cfg.get("max_peaks") or 150,
        min_peaks=15 if cfg.get("min_peaks") is None else cfg["min_peaks"],
        min_matched_peaks=4 if cfg.get("min_matched_peaks") is None else cfg["min_matched_peaks"],
        max_fragment_charge=cfg.get("max_fragment_charge"), annotate_matches=bool(cfg.get("annotate_matches", False)),
        precursor_charge=(int(pc[0]), int(pc[1])), override_precursor_charge=bool(cfg.get("override_precursor_charge", False)),
        isotope_errors=(int(iso[0]), int(iso[1])), deisotope=True if cfg.get("deisotope") is None else bool(cfg["deisotope"]),
        chimera=bool(cfg.get("chimera", False)), wide_window=bool(cfg.get("wide_window", False)),
        score_type=cfg.get("score_type") or "SageHyperScore",
        predict_rt=True if cfg.get("predict_rt") is None else bool(cfg["predict_rt"]),  # input.rs:372
        protein_grouping=True if cfg.get("protein_grouping") is None else bool(cfg["protein_grouping"]),  # input.rs:382
        protein_grouping_peptide_fdr=0.01 if cfg.get("protein_grouping_peptide_fdr") is None
        else float(cfg["protein_grouping_peptide_fdr"]),  # input.rs:383
        # the protein-group stage runs when the configuration names one of its keys (see run())
        protein_group_stage=cfg.get("protein_grouping") is not None or cfg.get("protein_grouping_peptide_fdr") is not None)


def quant_settings(cfg: dict, log=print):
    """QuantOptions -> QuantSettings (input.rs:87-133, 168-196): (lfq, LfqSettings).  `lfq` defaults to false; every absent
    lfq_settings key takes LfqSettings::default (lfq.rs:56-68); spectral_angle and ppm_tolerance are taken as absolute values;
    the strategies are the enum variant names ("Hybrid", "Sum", ...).  The warnings of input.rs:113-130 go to `log`."""
    q = cfg.get("quant") or {}
    on = bool(q.get("lfq")) if q.get("lfq") is not None else False
    o = q.get("lfq_settings") or {}
    d = LfqSettings()
    pick = lambda k: d.__dict__[k] if o.get(k) is None else o[k]
    st = LfqSettings(peak_scoring=pick("peak_scoring"), integration=pick("integration"),
                     spectral_angle=abs(float(pick("spectral_angle"))), ppm_tolerance=abs(float(pick("ppm_tolerance"))),
                     mobility_pct_tolerance=float(pick("mobility_pct_tolerance")),
                     combine_charge_states=bool(pick("combine_charge_states")), peptide_q_value=float(pick("peptide_q_value")))
    if st.peak_scoring not in LFQ_SCORING:
        raise SystemExit(f"quant.lfq_settings.peak_scoring: unknown variant `{st.peak_scoring}`, expected one of "
                         + ", ".join(f"`{v}`" for v in LFQ_SCORING))
    if st.integration not in LFQ_INTEGRATION:
        raise SystemExit(f"quant.lfq_settings.integration: unknown variant `{st.integration}`, expected one of "
                         + ", ".join(f"`{v}`" for v in LFQ_INTEGRATION))
    if st.ppm_tolerance > 20.0:
        log("lfq_settings.ppm_tolerance is higher than expected")
    if st.mobility_pct_tolerance > 4.0:
        log("lfq_settings.mobility_pct_tolerance is higher than expected")
    if st.mobility_pct_tolerance < 0.05:
        log("lfq_settings.mobility_pct_tolerance is smaller than expected")
    if st.spectral_angle < 0.50:
        log("lfq_settings.spectral_angle is lower than expected")
    if st.peptide_q_value > 0.01:
        log("lfq_settings.peptide_q_value is higher than expected, expect increased runtime and memory usage")
    if st.peptide_q_value < 0.01:
        log("lfq_settings.peptide_q_value is lower than expected, not all identified peptides will have MS1 intensities extracted")
    return on, st


def protein_lfq_settings(cfg: dict):
    """quant.protein_lfq / quant.protein_lfq_settings — an addition over the reference, whose serde structs ignore the keys
    (DESIGN.md 7g): (on, {"min_ratio_count", "precursor_q_value"}).  The roll-up reads lfq.tsv's rows, so it needs quant.lfq."""
    q = cfg.get("quant") or {}
    on = bool(q.get("protein_lfq")) if q.get("protein_lfq") is not None else False
    o = q.get("protein_lfq_settings") or {}
    st = {"min_ratio_count": 1 if o.get("min_ratio_count") is None else int(o["min_ratio_count"]),
          "precursor_q_value": 0.05 if o.get("precursor_q_value") is None else float(o["precursor_q_value"])}
    if st["min_ratio_count"] < 0:
        raise SystemExit("quant.protein_lfq_settings.min_ratio_count must not be negative")
    if on and not (q.get("lfq") is not None and bool(q.get("lfq"))):
        raise SystemExit("`quant.protein_lfq: true` needs `quant.lfq: true`: the protein roll-up reads the precursor areas of lfq.tsv")
    return on, st


def tmt_rollup_settings(cfg: dict, n_files=None):
    """quant.tmt_rollup / quant.tmt_rollup_settings — an addition over the reference, whose serde structs ignore the keys
    (DESIGN.md 7i): (on, {"by", "summary", "normalise", "psm_q_value", "min_channels", "min_purity", "plex_of_file"}).  The roll-up
    reads tmt.tsv's rows, so it needs quant.tmt; min_purity reads purity.sage.tsv's column, so it needs precursor_purity.  n_files:
    the number of input files, when known (plex_of_file names the plex of each)."""
    q = cfg.get("quant") or {}
    on = bool(q.get("tmt_rollup")) if q.get("tmt_rollup") is not None else False
    o = q.get("tmt_rollup_settings") or {}
    pick = lambda k, d: d if o.get(k) is None else o[k]
    st = {"by": pick("by", "protein"), "summary": pick("summary", "Sum"), "normalise": pick("normalise", "Total"),
          "psm_q_value": float(pick("psm_q_value", 0.01)), "min_channels": int(pick("min_channels", 1)),
          "min_purity": None if o.get("min_purity") is None else float(o["min_purity"]),
          "plex_of_file": None if o.get("plex_of_file") is None else [int(x) for x in o["plex_of_file"]]}
    for key, allowed in (("by", ("protein", "peptide")), ("summary", ("Sum", "Median")), ("normalise", ("Total", "None"))):
        if st[key] not in allowed:
            raise SystemExit(f"quant.tmt_rollup_settings.{key}: unknown variant `{st[key]}`, expected one of "
                             + ", ".join(f"`{v}`" for v in allowed))
    if st["min_channels"] < 0:
        raise SystemExit("quant.tmt_rollup_settings.min_channels must not be negative")
    if st["plex_of_file"] is not None and any(x < 0 for x in st["plex_of_file"]):
        raise SystemExit("quant.tmt_rollup_settings.plex_of_file must not hold negative plex ids")
    if on and q.get("tmt") is None:
        raise SystemExit("`quant.tmt_rollup: true` needs `quant.tmt`: the roll-up reads the reporter intensities of tmt.tsv")
    if on and st["min_purity"] is not None and not bool(cfg.get("precursor_purity", False)):
        raise SystemExit("`quant.tmt_rollup_settings.min_purity` needs `precursor_purity: true`: the filter reads the purity of "
                         "purity.sage.tsv")
    if on and n_files is not None and st["plex_of_file"] is not None and len(st["plex_of_file"]) != n_files:
        raise SystemExit(f"quant.tmt_rollup_settings.plex_of_file names {len(st['plex_of_file'])} files, the run has {n_files}")
    return on, st


def purity_settings(cfg: dict):
    """precursor_purity / purity_settings, top-level keys — an addition over the reference, whose serde schema ignores them
    (DESIGN.md 7h): (on, {"ppm_tolerance", "max_isotope", "default_isolation"})."""
    on = bool(cfg.get("precursor_purity", False))
    o = cfg.get("purity_settings") or {}
    iso = o.get("default_isolation")
    st = {"ppm_tolerance": 10.0 if o.get("ppm_tolerance") is None else float(o["ppm_tolerance"]),
          "max_isotope": 4 if o.get("max_isotope") is None else int(o["max_isotope"]),
          "default_isolation": (-0.5, 0.5) if iso is None else (float(iso[0]), float(iso[1]))}
    if not (0.0 <= st["ppm_tolerance"] < float("inf")):
        raise SystemExit("purity_settings.ppm_tolerance must be finite and not negative")
    if not 0 <= st["max_isotope"] <= 16:
        raise SystemExit("purity_settings.max_isotope must be between 0 and 16")
    return on, st


def tmt_settings(cfg: dict, log=print):
    """quant.tmt / quant.tmt_settings (input.rs:136-196): (Isobaric or None, TmtSettings).  `tmt` is the externally tagged
    enum ("Tmt6" | "Tmt10" | "Tmt11" | "Tmt16" | "Tmt18" | {"User": [..]}); level defaults to 3, sn to false.  The level
    warning of runner.rs:347-349 goes to `log`."""
    q = cfg.get("quant") or {}
    o = q.get("tmt_settings") or {}
    d = TmtSettings()
    st = TmtSettings(level=d.level if o.get("level") is None else int(o["level"]), sn=d.sn if o.get("sn") is None else bool(o["sn"]))
    if q.get("tmt") is None:
        return None, st
    try:
        iso = Isobaric.from_json(q["tmt"])
    except ValueError as e:
        raise SystemExit(f"quant.tmt: {e}")
    if st.level not in (2, 3):
        log(f"TMT quant level set at {st.level}, is this correct?")
    return iso, st


def scorer_params(sp: dict) -> ScorerParams:
    """The Scorer struct literal of runner.rs:492-508."""
    return ScorerParams(precursor_tol=sp["precursor_tol"], fragment_tol=sp["fragment_tol"],
                        min_matched_peaks=sp["min_matched_peaks"], min_isotope_err=sp["isotope_errors"][0],
                        max_isotope_err=sp["isotope_errors"][1], min_precursor_charge=sp["precursor_charge"][0],
                        max_precursor_charge=sp["precursor_charge"][1],
                        override_precursor_charge=sp["override_precursor_charge"], max_fragment_charge=sp["max_fragment_charge"],
                        chimera=sp["chimera"], report_psms=sp["report_psms"], wide_window=sp["wide_window"],
                        annotate_matches=sp["annotate_matches"], score_type=sp["score_type"])


def _upload(scorer, processor, raw, sp, host_preprocess, positions=False):
    """spectra of one file (RawBatch) -> resident ProcessedSpectrum batch (+ spectrum ids); None when nothing is left to search.
    positions=True: also the positions in `raw` of the spectra the batch holds."""
    kinds = getattr(raw, "iso_kind", None)  # (searchable: the window kinds of an MGF file with ppm windows; None: all Da)
    if host_preprocess:  # SpectrumProcessor::process on the host (C++), spectra below min_peaks dropped (runner.rs:313)
        processed = [(i, processor.process(raw.spectrum(i))) for i in range(raw.n)]
        processed = [(i, p) for i, p in processed if len(p.masses) >= sp["min_peaks"]]
        if not processed:
            return (None, [], np.zeros(0, np.int64)) if positions else (None, [])
        pos = np.array([i for i, _ in processed], dtype=np.int64)
        out = (scorer.upload(SpectrumBatch.from_spectra([p for _, p in processed]), iso_kind=None if kinds is None else kinds[pos]),
               [p.id for _, p in processed])
        return out + (pos,) if positions else out
    # ... or on the device: raw peaks in, PSMs out; spectra below min_peaks stay in the batch with zero peaks
    dbatch, _ = scorer.process_upload(raw, sp["max_peaks"], sp["deisotope"], processor.min_deisotope_mz, sp["min_peaks"], iso_kind=kinds)
    return (dbatch, list(raw.ids), np.arange(raw.n, dtype=np.int64)) if positions else (dbatch, list(raw.ids))


def searchable(raw, kinds, charge_zero, sp, path, quantified=False):
    """The spectra of one file (read_spectra) that the search scores.  MGF input carries two things an mzML run never does:
    * the kind of each isolation window (`TOLU=ppm`), which only the wide-window search reads (scoring.rs:427-431): kept as
      `raw.iso_kind` when some window is not in Da, for the `_kinds` upload entry points;
    * charge 0 annotated on precursors[0] (`CHARGE=0`): the reference searches around mass 0 in a narrow search and reports no
      PSM (scoring.rs:439-443), so those spectra are left out.  Where the charge is ignored (wide window, override) they are
      searched, but deisotoping would use a maximum charge of 0 (spectrum.rs:289-293), which this build does not do: refused
      (check_inputs, before any work).
    quantified: the spectra are also TMT-quantified at level 2 (their deisotoping counts there too)."""
    if raw.n == 0:
        return raw
    zero = charge_zero.astype(bool)
    if zero.any():
        narrow = not sp["wide_window"] and not sp["override_precursor_charge"]
        if sp["deisotope"] and (not narrow or quantified):
            raise SystemExit(f"{path}: precursor charge 0 with deisotoping is not supported by this build")
        if narrow:
            keep = np.flatnonzero(~zero)
            raw, kinds = raw.subset(keep), kinds[keep]
    if (kinds != TOL_DA).any():
        raw.iso_kind = np.ascontiguousarray(kinds, dtype=np.uint8)
    return raw


def check_inputs(paths, sp, quantified):
    """Refuse up front, before any device work, what searchable() would refuse in a later file: precursor charge 0 of an MGF
    spectrum where deisotoping would use it."""
    narrow = not sp["wide_window"] and not sp["override_precursor_charge"]
    if not sp["deisotope"] or (narrow and not quantified):
        return
    for path in paths:
        if is_mgf(path) and read_mgf_native(path)[2].any():
            raise SystemExit(f"{path}: precursor charge 0 with deisotoping is not supported by this build")


def prefilter_peptides(dbp, fasta_text, chunk, n_targets, sp, mzml_paths, processor, device, host_preprocess, log, sn_level=None):
    """Runner::prefilter_peptides (runner.rs:143-238): search every spectrum against the FASTA one chunk of target proteins
    at a time with Scorer::quick_score, keep the peptides some spectrum picked, merge the survivors (reorder_peptides) and
    leave build_from_peptides to the device.  The scorer of this pass reports one PSM more than the final one (runner.rs:190).
    sn_level: the MS2 intensities are divided by their noise (TMT `sn` at level 2; the pass reads as the search does)."""
    raws = [searchable(*read_spectra(path, file_id=file_id, ms_level=2, sn_level=sn_level), sp, path)
            for file_id, path in enumerate(mzml_paths)]
    pass_params = scorer_params(dict(sp, report_psms=sp["report_psms"] + 1))
    chunks, keeps = [], []
    for chunk_id, first in enumerate(range(0, n_targets, chunk)):
        t0 = time.time()
        log(f"pre-filtering fasta chunk {chunk_id}")
        cdb = dbp.build_chunk(fasta_text, first, chunk, peptides_only=True)
        keep = np.zeros(cdb.n_peptides, dtype=np.uint8)
        if cdb.n_peptides:
            scorer = Scorer(DeviceDatabase(cdb, device), pass_params)
            n = 0
            for raw in raws:
                if raw.n == 0:
                    continue
                dbatch, _ = _upload(scorer, processor, raw, sp, host_preprocess)
                if dbatch is None:
                    continue
                scorer.quick_score(dbatch, True if dbp.prefilter_low_memory is None else bool(dbp.prefilter_low_memory), keep)
                n += dbatch.n
                dbatch.close()
            dt = (time.time() - t0) * 1000.0
            log(f"- prefilter search:  {int(dt):8d} ms ({int(n * 1000 / (dt + 1))} spectra/s)")  # runner.rs:272-277
        log(f"found {int(keep.sum())} pre-filtered peptides for fasta chunk {chunk_id}")
        chunks.append(cdb)
        keeps.append(keep)
    return dbp.merge_kept(chunks, keeps, peptides_only=True)


def read_text(path: str) -> str:
    """FASTA text; gzip-compressed files (sage-cloudpath lib.rs:44-90 gunzips `*.gz` / `*.gzip`; here: by the 1f 8b magic)."""
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        import gzip
        raw = gzip.decompress(raw)
    return raw.decode()


def parse_devices(spec, n_visible: int):
    """--devices all | 0-7 | 0,2,3 (a device may be named twice: two workers share it, on one copy of the index)"""
    if spec is None:
        return None
    if spec == "all":
        return list(range(n_visible))
    out = []
    try:
        for part in str(spec).split(","):
            if "-" in part:
                a, b = part.split("-")
                out += list(range(int(a), int(b) + 1))
            else:
                out.append(int(part))
    except ValueError:
        raise SystemExit(f"sage_amd.cli: --devices {spec}: expected `all`, a list like 0,2,3 or a range like 0-7")
    bad = [d for d in out if d < 0 or d >= n_visible]
    if bad or not out:
        raise SystemExit(f"sage_amd.cli: --devices {spec}: {n_visible} HIP device(s) visible")
    return out


NO_ISOMER = 0xFFFFFFFF


def isomer_candidates(groups, feats, counts):
    """The candidate lists of Scorer.score_candidates for isomer scoring: for every reported PSM (slot i * report_psms + r,
    r < counts[i]) every OTHER member of its peptide's isomer group, ascending.  groups: IndexedDatabase.isomer_groups().
    Returns (cand_off[n * report_psms + 1] u64, cand_pep u32)."""
    group_of, group_off, members = groups
    n, report = feats.shape
    valid = (np.arange(report)[None, :] < np.asarray(counts)[:, None]).reshape(-1)
    pep = feats["peptide_idx"].reshape(-1).astype(np.int64)
    g = np.where(valid, group_of[np.where(valid, pep, 0)] if len(group_of) else NO_ISOMER, NO_ISOMER).astype(np.int64)
    has = g != NO_ISOMER
    first = np.zeros(n * report, dtype=np.int64)
    size = np.zeros(n * report, dtype=np.int64)
    first[has] = group_off[g[has]].astype(np.int64)
    size[has] = group_off[g[has] + 1].astype(np.int64) - first[has]
    before = np.cumsum(size) - size
    mem = members[np.repeat(first - before, size) + np.arange(int(size.sum()))] if size.sum() else np.zeros(0, np.uint32)
    cand_pep = mem[mem != np.repeat(pep, size)].astype(np.uint32)
    cand_off = np.zeros(n * report + 1, dtype=np.uint64)
    cand_off[1:] = np.cumsum(np.where(has, size - 1, 0))
    return cand_off, cand_pep


def best_isomers(cand_off, cand_pep, scores):
    """Per slot: (number of candidates, the best one's peptide index, hyperscore, matched_b + matched_y) — the largest
    hyperscore under a plain f64 `>`, ties to the smallest peptide index (the lists are ascending); NO_ISOMER / 0 where a slot
    has no candidate."""
    off = cand_off.astype(np.int64)
    lens = np.diff(off)
    best_pep = np.full(len(lens), NO_ISOMER, dtype=np.uint32)
    best_h = np.zeros(len(lens), dtype=np.float64)
    best_m = np.zeros(len(lens), dtype=np.uint32)
    some = np.flatnonzero(lens > 0)
    if len(some):
        h = scores["hyperscore"]
        top = np.maximum.reduceat(h, off[some])
        at = np.where(h == np.repeat(top, lens[some]), np.arange(len(h)), len(h))
        pick = np.minimum.reduceat(at, off[some])
        best_pep[some], best_h[some] = cand_pep[pick], h[pick]
        best_m[some] = scores["matched_b"][pick] + scores["matched_y"][pick]
    return lens.astype(np.uint32), best_pep, best_h, best_m


def localisation_candidates(groups, feats, counts):
    """The candidate lists of Scorer.localise: for every reported PSM whose peptide has positional isomers, the PSM's own peptide
    followed by isomer_candidates' members.  Returns (cand_off[n * report_psms + 1] u64, cand_pep u32)."""
    off, others = isomer_candidates(groups, feats, counts)
    lens = np.diff(off.astype(np.int64))
    has = lens > 0
    cand_off = np.zeros(len(lens) + 1, dtype=np.uint64)
    cand_off[1:] = np.cumsum(lens + has)
    cand_pep = np.empty(int(cand_off[-1]), dtype=np.uint32)
    own_at = cand_off[:-1].astype(np.int64)[has]
    rest = np.ones(len(cand_pep), dtype=bool)
    rest[own_at] = False
    cand_pep[own_at] = feats["peptide_idx"].reshape(-1)[has]
    cand_pep[rest] = others
    return cand_off, cand_pep


def localisation_columns(cand_off, cand_pep, slots):
    """Per slot, from Scorer.localise's records: (placements, best placement's peptide index, its peptide score, the second one's
    peptide index, its peptide score, site-determining items, depth, ascore, reported_is_best); NO_ISOMER / 0 / NaN where a slot has
    no list.  The reported peptide is position 0 of its list."""
    off = cand_off.astype(np.int64)
    lens = np.diff(off)
    some = lens > 0
    best_pep = np.full(len(lens), NO_ISOMER, dtype=np.uint32)
    second_pep = np.full(len(lens), NO_ISOMER, dtype=np.uint32)
    best_pep[some] = cand_pep[off[:-1][some] + slots["best"][some].astype(np.int64)]
    pair = some & (slots["second"] != NO_ISOMER)
    second_pep[pair] = cand_pep[off[:-1][pair] + slots["second"][pair].astype(np.int64)]
    return (lens.astype(np.uint32), best_pep, slots["best_score"].copy(), second_pep, slots["second_score"].copy(),
            slots["n_site_items"].copy(), slots["depth"].copy(), slots["ascore"].copy(), some & (slots["best"] == 0))


def search_file(workers, processor, raw, sp, host_preprocess, annotate, pep_mono=None, isomers=None, localise=None):
    """Scorer::score over every MS2 spectrum of one file (runner.rs:311-325), on all the workers' devices at once: the file's
    spectra are cut into work-balanced shards that are contiguous in PRECURSOR MASS (sharding.plan_mass_shards: index
    replicated, no exchange between devices, and a device walks 1 / N of the mass-sorted index instead of all of it), one host
    thread per device preprocesses, scores and — if asked — annotates its shard, and the shards' results are merged back into
    input order, as `collect()` leaves them.  Returns (features[n, report], counts[n], ids, annotation | None).
    isomers: IndexedDatabase.isomer_groups() — each shard's device then scores the positional isomers of its PSMs next to the
    annotation call, and a fifth value is returned: (isomers, best_isomer peptide, isomer_hyperscore, isomer_matched_peaks),
    each [n, report] (best_isomers).
    localise: the same table — each shard's device then localises the modification sites of its PSMs (Scorer.localise over
    localisation_candidates), and a sixth value is returned: localisation_columns' arrays, each [n, report].  With either of the
    two asked for, six values are returned, None in the place of the one that was not."""
    import threading

    from .sharding import estimate_work, plan_mass_shards, plan_shards, precursor_sort_mass
    shards = [np.arange(raw.n, dtype=np.int64)]
    if len(workers) > 1:
        # work per spectrum ~ peaks x queries x candidates in the precursor window (precursor mass drifts with retention time, and
        # in an open search the window size spans orders of magnitude): sharding.estimate_work
        params = scorer_params(sp)
        if pep_mono is None:  # (no masses to estimate windows from: contiguous ranges of the file, balanced on peak counts)
            shards = [np.arange(b, e, dtype=np.int64) for b, e in plan_shards(raw.peak_off, len(workers))]
        else:
            # eight blocks of the mass axis per device, every len(workers)-th block each: the window sizes of an open search span
            # orders of magnitude ALONG the mass axis, so within a block the estimate's weights still matter
            iso_lo, iso_hi = raw.isolation_lo, raw.isolation_hi
            if getattr(raw, "iso_kind", None) is not None or np.isinf(iso_lo).any():  # (MGF; weights only: ppm windows as Da
                ppm = raw.iso_kind != TOL_DA if getattr(raw, "iso_kind", None) is not None else np.zeros(raw.n, bool)  # around m/z,
                iso_lo = np.where(ppm, iso_lo * raw.precursor_mz * np.float32(1e-6), iso_lo)  # the empty windows of TOL=NaN as 0)
                iso_hi = np.where(ppm, iso_hi * raw.precursor_mz * np.float32(1e-6), iso_hi)
                iso_lo, iso_hi = np.where(np.isinf(iso_lo), 0, iso_lo), np.where(np.isinf(iso_hi), 0, iso_hi)
            weights = estimate_work(raw.peak_off, raw.precursor_mz, raw.precursor_charge, params, pep_mono, iso_lo, iso_hi)
            narrow = not params.wide_window and params.precursor_tol.kind != "da"
            shards = plan_mass_shards(precursor_sort_mass(raw.precursor_mz, raw.precursor_charge, params), len(workers),
                                      None if narrow else weights)
    results = [None] * len(workers)
    stage_ms = [(0.0, 0.0, 0.0, 0.0, 0.0)] * len(workers)  # per worker: preprocess + upload, score, annotate, isomers, localisation
    errors = []

    def work(k):
        try:
            idx = shards[k]
            scorer = workers[k][1]
            part = raw if len(idx) == raw.n else raw.subset(idx)
            if part is not raw and getattr(raw, "iso_kind", None) is not None:
                part.iso_kind = raw.iso_kind[idx]
            if part.n == 0:
                return
            t0 = time.time()
            dbatch, ids, kept = _upload(scorer, processor, part, sp, host_preprocess, positions=True)
            if dbatch is None:
                return
            t1 = time.time()
            feats, counts = scorer.score_resident(dbatch)
            feats, counts = feats.copy(), counts.copy()
            t2 = time.time()
            ann = scorer.annotate(dbatch, feats, counts) if annotate else None
            t3 = time.time()
            iso = None
            if isomers is not None:
                cand_off, cand_pep = isomer_candidates(isomers, feats, counts)
                iso = tuple(a.reshape(feats.shape) for a in
                            best_isomers(cand_off, cand_pep, scorer.score_candidates(dbatch, feats, counts, cand_off, cand_pep)))
            t4 = time.time()
            loc = None
            if localise is not None:
                cand_off, cand_pep = localisation_candidates(localise, feats, counts)
                loc = tuple(a.reshape(feats.shape) for a in
                            localisation_columns(cand_off, cand_pep, scorer.localise(dbatch, feats, counts, cand_off, cand_pep)))
            dbatch.close()
            stage_ms[k] = ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (time.time() - t4) * 1e3)
            results[k] = (feats, counts, ids, ann, idx[kept], iso, loc)  # (idx[kept]: positions in the file of the batch's spectra)
        except BaseException as exc:  # noqa: BLE001 — re-raised on the calling thread
            errors.append(exc)

    if len(workers) == 1:
        work(0)
    else:
        ts = [threading.Thread(target=work, args=(k,)) for k in range(len(workers))]
        [t.start() for t in ts]
        [t.join() for t in ts]
    if errors:
        raise errors[0]
    parts = [r for r in results if r is not None]
    if not parts:
        return None
    # merge: rows in the order of their spectra's positions in the file (one part: already so)
    feats = np.concatenate([p[0] for p in parts], axis=0)
    counts = np.concatenate([p[1] for p in parts])
    ids = [i for p in parts for i in p[2]]
    where = np.concatenate([p[4] for p in parts])
    perm = np.argsort(where, kind="stable")
    report = feats.shape[1]
    ann = None
    if annotate:  # Fragments: one run per PSM slot, offsets per part — gather the runs in the merged slot order
        lens = np.concatenate([np.diff(p[3][0].astype(np.int64)) for p in parts])  # per slot (rows x report), concatenated parts
        starts = np.concatenate([p[3][0][:-1].astype(np.int64) + b for p, b in
                                 zip(parts, np.cumsum([0] + [int(p[3][0][-1]) for p in parts[:-1]]))])
        slot = (perm[:, None] * report + np.arange(report)[None, :]).reshape(-1)
        new_off = np.zeros(len(slot) + 1, dtype=np.uint64)
        new_off[1:] = np.cumsum(lens[slot])
        gather = np.repeat(starts[slot] - new_off[:-1].astype(np.int64), lens[slot]) + np.arange(int(new_off[-1]))
        ann = (new_off, {k: np.concatenate([p[3][1][k] for p in parts])[gather] for k in parts[0][3][1]})
    feats, counts, ids = feats[perm], counts[perm], [ids[i] for i in perm]
    valid = np.arange(report)[None, :] < counts[:, None]
    feats["spec_index"] = np.where(valid, np.arange(len(counts), dtype=np.uint32)[:, None], feats["spec_index"])  # row of `ids`
    search_file.last_stage_ms = tuple(max(x[i] for x in stage_ms) for i in range(3))  # (the slowest worker's, per stage)
    if isomers is not None or localise is not None:
        search_file.last_isomer_ms = max(x[3] for x in stage_ms)
        search_file.last_localise_ms = max(x[4] for x in stage_ms)

        def merged(at):
            return tuple(np.concatenate([p[at][j] for p in parts], axis=0)[perm] for j in range(len(parts[0][at])))
        return feats, counts, ids, ann, merged(5) if isomers is not None else None, merged(6) if localise is not None else None
    return feats, counts, ids, ann


def run(cfg: dict, mzml_paths, output_directory: str, device: int = 0, log=print, host_preprocess: bool = False,
        write_pin: bool = False, devices=None) -> dict:
    if device_count() <= 0:
        raise SystemExit("sage_amd.cli: no HIP device visible — libsage_hip has no CPU fallback")
    sp = search_parameters(cfg)
    lfq_on, lfq_settings = quant_settings(cfg, log)
    protein_lfq_on, protein_lfq_st = protein_lfq_settings(cfg)
    isobaric, tmt_st = tmt_settings(cfg, log)
    purity_on, purity_st = purity_settings(cfg)
    tmt_rollup_on, tmt_rollup_st = tmt_rollup_settings(cfg, len(list(mzml_paths)))
    # runner.rs:391-410: S/N division at the quant level; at level 2 the reporter region is kept out of deisotoping
    sn_level = tmt_st.level if (isobaric is not None and tmt_st.sn) else None
    ms2_sn = sn_level if sn_level == 2 else None
    cutoff = isobaric.min_deisotope_mz() if (isobaric is not None and tmt_st.level == 2) else 0.0
    if lfq_on and not sp["predict_rt"]:  # input.rs:309-316
        log("`predict_rt: false` and `lfq: true` are incompatible. Setting `predict_rt: true`")
        sp["predict_rt"] = True
    dbp = DatabaseParameters.from_json(cfg["database"])
    if not dbp.fasta:
        raise SystemExit("`database.fasta` must be set. For more information try '--help'")
    # (any report_psms the library takes: lists of max(50, 2 * report_psms) candidates live in LDS while they fit a compute unit,
    # in a global-memory workspace beyond — capi.hip: enqueue_compute; the prefilter pass scores with report_psms + 1)
    need = sp["report_psms"] + (1 if dbp.prefilter else 0)
    if need > 32767:
        raise SystemExit(f"sage_amd.cli: report_psms = {sp['report_psms']}: this build supports report_psms <= 32767")
    devices = list(devices) if devices else [device]
    device = devices[0]
    t0 = time.time()
    check_inputs(list(mzml_paths), sp, isobaric is not None and tmt_st.level == 2)
    fasta_text = read_text(dbp.fasta)
    params = scorer_params(sp)
    processor = SpectrumProcessor(sp["max_peaks"], sp["deisotope"], cutoff)
    host = None
    if dbp.prefilter:  # runner.rs:104-127
        chunk = dbp.auto_prefilter_chunk_size(fasta_text)
        n_targets = dbp.num_targets(fasta_text)
        if chunk < n_targets:
            log(f"using {(n_targets + chunk - 1) // chunk} db chunks of size {chunk}")
            host = prefilter_peptides(dbp, fasta_text, chunk, n_targets, sp, mzml_paths, processor, device, host_preprocess, log,
                                      sn_level=ms2_sn)
    if host is None:
        host = dbp.build(fasta_text, peptides_only=True)  # digest / modify / sort / dedup on the host ...
    # ... build_from_peptides on the device (index_build.hip): the index is replicated on every device that searches
    workers, first = [], {}
    for d in devices:  # one copy of the index per distinct device; a device named again gets a second handle on it
        if d in first:
            workers.append((first[d][0], first[d][1].clone()))  # (sage_hip_scorer_clone: own streams and working set)
        else:
            dev_db = DeviceDatabase(host, d)
            first[d] = (dev_db, Scorer(dev_db, params))
            workers.append(first[d])
    log(f"generated {host.n_peptides} peptides and their fragment index in {int((time.time() - t0) * 1000)}ms" +
        (f" on {len(devices)} devices" if len(devices) > 1 else ""))
    os.makedirs(output_directory, exist_ok=True)
    # "score_isomers": an addition over the reference, whose serde schema ignores the key.  The table of positional isomers is made
    # once per run, on the host threads; every file's PSMs are then scored against their isomers on the device that holds the batch
    isomer_groups, isomer_parts, isomer_ms = None, [], 0.0
    if bool(cfg.get("score_isomers", False)):
        t_iso = time.time()
        isomer_groups = host.isomer_groups()
        isomer_ms = (time.time() - t_iso) * 1e3
    # "localise": likewise an addition, over the same table; on its own or next to "score_isomers"
    localise_groups, localise_parts, localise_ms = None, [], 0.0
    if bool(cfg.get("localise", False)):
        t_loc = time.time()
        localise_groups = host.isomer_groups()
        localise_ms = (time.time() - t_loc) * 1e3
    feats_all, meta, frags = [], [], []  # per PSM: (filename, spectrum id); matched-fragment rows
    psm_id = 1  # PSM_COUNTER starts at 1 (scoring.rs:163)
    n_searched = 0
    search_ms = 0.0
    stage_totals = {"file_io_ms": 0.0, "preprocess_upload_ms": 0.0, "score_ms": 0.0, "annotate_ms": 0.0}
    t_run = time.time()
    # The reader works one file ahead of the search (the reference reads and preprocesses its files in parallel batches,
    # runner.rs:450-461): file k + 1 is parsed on the host threads (csrc/mzml_reader.cpp decodes the spectra of a file in
    # parallel, outside the GIL) while the devices score file k.
    from concurrent.futures import ThreadPoolExecutor

    def read_file(file_id, path):
        t0 = time.time()
        # (read_spectra: .mgf / .mgf.gz to the MGF reader, which has MS2 only and no S/N option; anything else as mzML)
        raw = read_spectra(path, file_id=file_id, ms_level=2, check_searchable=True, sn_level=ms2_sn)
        ms1 = read_spectra(path, file_id=file_id, ms_level=1)[0] if lfq_on or purity_on else None  # (runner.rs:361-363: only for LFQ; 7h)
        # TMT at a level other than 2 (SPS-MS3): that level's spectra (level 1 quantifies nothing: tmt.rs:330)
        msn = (read_spectra(path, file_id=file_id, ms_level=tmt_st.level, sn_level=sn_level)[0]
               if isobaric is not None and tmt_st.level not in (1, 2) else None)
        search = searchable(*raw, sp, path, quantified=isobaric is not None and tmt_st.level == 2)
        return raw[0], search, ms1, msn, (time.time() - t0) * 1000.0

    mzml_paths = list(mzml_paths)
    ms1_batches = []
    purity_parts = []  # per file: (precursor m/z, isolation_lo, isolation_hi, scan start time) of every PSM's spectrum
    tmt_parts, tmt_ms = [], 0.0  # per file: (file_id, spectrum ids, ion injection times, intensities[n, labels])
    reader = ThreadPoolExecutor(max_workers=1)
    ahead = reader.submit(read_file, 0, mzml_paths[0]) if mzml_paths else None
    for file_id, path in enumerate(mzml_paths):
        try:
            raw, search_raw, ms1, msn, io_ms = ahead.result()
        except BaseException:
            reader.shutdown(wait=True)
            raise
        ahead = reader.submit(read_file, file_id + 1, mzml_paths[file_id + 1]) if file_id + 1 < len(mzml_paths) else None
        log(f"- file IO: {int(io_ms):8d} ms")
        if ms1 is not None and ms1.n:
            ms1_batches.append(ms1)
        if isobaric is not None and tmt_st.level != 1:  # tmt::quantify per file, on the first device (runner.rs:334-359)
            t0 = time.time()
            q = raw if tmt_st.level == 2 else msn
            if q.n:
                res = tmt([q], isobaric, tmt_st.level, sp["max_peaks"], sp["deisotope"], cutoff, device=device)
                tmt_parts.append((file_id, list(q.ids) if tmt_st.level == 2 else list(q.precursor_ref), q.ion_injection_time,
                                  res.intensity))
            tmt_ms += (time.time() - t0) * 1000.0
        if search_raw.n == 0:
            continue
        t0 = time.time()
        found = search_file(workers, processor, search_raw, sp, host_preprocess, sp["annotate_matches"], host.pep_mono,
                            isomers=isomer_groups, localise=localise_groups)
        if found is None:
            continue
        feats, counts, ids, ann = found[:4]
        n_batch = len(counts)
        dt = (time.time() - t0) * 1000.0
        search_ms += dt
        n_searched += n_batch
        log(f"- search:  {int(dt):8d} ms ({int(n_batch * 1000 / (dt + 1))} spectra/s)")  # runner.rs:327-330
        pre_ms, score_ms, ann_ms = getattr(search_file, "last_stage_ms", (0.0, 0.0, 0.0))
        log(f"    of which preprocessing + upload {pre_ms:.1f} ms, Scorer::score on the device {score_ms:.1f} ms" +
            (f", fragment annotation {ann_ms:.1f} ms" if sp["annotate_matches"] else ""))
        stage_totals["file_io_ms"] += io_ms
        stage_totals["preprocess_upload_ms"] += pre_ms
        stage_totals["score_ms"] += score_ms
        stage_totals["annotate_ms"] += ann_ms
        off, arr = ann if ann is not None else (None, None)
        name = os.path.basename(path)
        # the PSMs of the file in (spectrum, rank) order — the order Scorer::score results are collected in (runner.rs:325)
        spec_of = np.repeat(np.arange(n_batch), counts.astype(np.int64))
        rank_of = np.arange(len(spec_of)) - np.repeat(np.cumsum(counts.astype(np.int64)) - counts, counts.astype(np.int64))
        part = feats[spec_of, rank_of].copy()
        part["file_id"] = file_id
        feats_all.append(part)
        if isomer_groups is not None:
            isomer_parts.append(tuple(a[spec_of, rank_of] for a in found[4]))
            isomer_ms += getattr(search_file, "last_isomer_ms", 0.0)
        if localise_groups is not None:
            localise_parts.append(tuple(a[spec_of, rank_of] for a in found[5]))
            localise_ms += getattr(search_file, "last_localise_ms", 0.0)
        meta += [(psm_id + j, name, ids[i]) for j, i in enumerate(spec_of.tolist())]
        if purity_on:
            at = {s: k for k, s in enumerate(search_raw.ids)}
            row = np.array([at[ids[i]] for i in spec_of.tolist()], dtype=np.int64)
            purity_parts.append((search_raw.precursor_mz[row], search_raw.isolation_lo[row], search_raw.isolation_hi[row],
                                 search_raw.scan_start_time[row]))
        if arr is not None:
            for j, (i, r) in enumerate(zip(spec_of.tolist(), rank_of.tolist())):
                slot = i * params.report_psms + r
                frags.append(output.fragment_rows(psm_id + j, int(off[slot]), int(off[slot + 1]), arr))
        psm_id += len(part)
    reader.shutdown(wait=True)
    # runner.rs:536-541: spectrum_fdr (LDA or heuristic, sort, q-values), picked_peptide, picked_protein — on the device.
    # runner.rs:539-549: generate_protein_groups + picked_protein_group, when the configuration names `protein_grouping` or
    # `protein_grouping_peptide_fdr` (the reference runs the block in every run; here a configuration without either key keeps the
    # columns' defaults, so that its results.sage.tsv stays the file sage_hip_write_results writes for a caller of the C ABI that
    # does not call sage_hip_protein_groups)
    flat = np.concatenate(feats_all) if feats_all else np.zeros(0, dtype=L_FEATURE_DTYPE)
    post = None
    rtp = None
    groups = None
    order = range(len(flat))
    rescore_summary = {}
    if len(flat):
        t0 = time.time()
        model_inputs = {}
        if sp["predict_rt"]:  # runner.rs:513-530: poisson-sorted q-values, global_alignment, retention / mobility models
            off, seq, mono = host.feature_peptides(flat["peptide_idx"])
            rtp = predict_rt(flat, len(mzml_paths), off, seq, mono, device=device)
            for a in rtp.alignments:
                log(f"aligning file #{int(a['file_id'])}: y = {float(a['slope']):.4f}x + {float(a['intercept']):.4f}")
            log(f"aligned retention times across {len(mzml_paths)} files")
            if rtp.rt_fitted:
                log(f"- fit retention time model, rsq = {rtp.rt_r2}")
            if rtp.ims_fitted:
                log(f"- fit mobility model, rsq = {rtp.ims_r2}")
            else:
                log("Mobility model failed to train")
            model_inputs = dict(aligned_rt=rtp.aligned_rt, delta_rt_model=rtp.delta_rt_model, delta_ims_model=rtp.delta_ims_model)
        pk, npk, prk, npr = host.competition_keys(flat["peptide_idx"])
        res = rescore(flat, sp["precursor_tol"], pk, npk, prk, npr, device=device, **model_inputs)
        if not res.lda_fitted:
            log("linear model fitting failed, falling back to heuristic discriminant score")  # runner.rs:285
        post = res
        order = [int(i) for i in res.order]
        log(f"discovered {res.passing_spectrum} target peptide-spectrum matches at 1% FDR")  # runner.rs:576-587
        log(f"discovered {res.passing_peptide} target peptides at 1% FDR")
        log(f"discovered {res.passing_protein} target proteins (supported by proteotypic peptides only) at 1% FDR")
        group_summary = {}
        if sp["protein_group_stage"]:
            groups = protein_groups(host, flat, res.peptide_q, res.discriminant_score, sp["protein_grouping"],
                                    sp["protein_grouping_peptide_fdr"], device=device)
            log(f"discovered {groups.passing_protein_group} target protein groups (supported by proteotypic peptides only) at 1% FDR")
            group_summary = {"q_protein_group": groups.passing_protein_group, "protein_groups": groups.n_groups,
                             "meta_peptides": groups.n_meta_peptides, "cover_rounds": groups.cover_rounds,
                             "protein_groups_device_ms": groups.device_ms}
        rescore_summary = {"lda_fitted": res.lda_fitted, "q_spectrum": res.passing_spectrum, "q_peptide": res.passing_peptide,
                           "q_protein": res.passing_protein, **group_summary, "rescore_ms": (time.time() - t0) * 1000.0,
                           "rescore_device_ms": res.device_ms}

    if rescore_summary:
        log(f"- rescoring (RT / IM models, LDA, q-values, picked FDR): {int(rescore_summary['rescore_ms']):8d} ms")
    lfq_result, lfq_summary = None, {}
    if lfq_on and rtp is not None:  # runner.rs:562-575: only when the alignments exist
        t0 = time.time()
        if not ms1_batches:
            log("no MS1 spectra found for quantification")  # lfq.rs:233
        carbon, sulfur = peptide_compositions(host.seq_off, host.seq)
        # MS1 spectra with a per-peak ion-mobility array (timsTOF mzML): sage_hip_lfq_im, which reads the features' `ims` and
        # lfq_settings.mobility_pct_tolerance (lfq.rs:111-127, 267-286); without one in any file, sage_hip_lfq as before
        with_mobility = any(b.mobility is not None for b in ms1_batches)
        lfq_result = lfq(flat, post.order, rtp.aligned_rt, post.peptide_q, rtp.alignments, ms1_batches, carbon, sulfur,
                         lfq_settings, sp["precursor_charge"], device=device, ion_mobility=with_mobility)
        log(f"discovered {lfq_result.passing} target MS1 peaks at 5% FDR")
        lfq_ms = (time.time() - t0) * 1000.0
        log(f"- label-free quantification: {int(lfq_ms):8d} ms")
        lfq_summary = {"q_precursor": lfq_result.passing, "lfq_grids": len(lfq_result.peptide_idx),
                       "lfq_windows": lfq_result.n_windows, "lfq_ms": lfq_ms, "lfq_device_ms": lfq_result.stage_ms["device_ms"],
                       "lfq_stage_ms": lfq_result.stage_ms, "lfq_ion_mobility": with_mobility,
                       "alignments": [{k: float(a[k]) if k != "file_id" else int(a[k]) for k in a.dtype.names}
                                      for a in rtp.alignments]}
    # writers: C++ (sage_hip_write_results) — byte-identical to output.feature_row / pin_row, which tests/test_cli_io.py checks
    t_write = time.time()
    filenames = [os.path.basename(p) for p in mzml_paths]
    psm_ids = [m[0] for m in meta]
    spec_ids = [m[2] for m in meta]
    results = os.path.join(output_directory, "results.sage.tsv")
    output.write_results_native(results, "tsv", host, flat, list(order), psm_ids, filenames, spec_ids, [rtp, post], groups)
    paths = [results]
    if sp["annotate_matches"]:
        fp = os.path.join(output_directory, "matched_fragments.sage.tsv")
        output.write_fragments(fp, [r for i in order for r in frags[i]])
        paths.append(fp)
    isomer_summary = {}
    if isomer_groups is not None:
        ip = os.path.join(output_directory, "isomers.sage.tsv")
        cols = [np.concatenate([p[j] for p in isomer_parts]) if isomer_parts else np.zeros(0) for j in range(4)]
        rows = output.isomer_rows(host, flat, list(order), psm_ids, *cols)
        output.write_isomers(ip, rows)
        paths.append(ip)
        isomer_summary = {"isomer_rows": len(rows), "isomer_ms": isomer_ms}
        log(f"- isomer scoring: {int(isomer_ms):8d} ms ({len(rows)} PSMs with positional isomers)")
    localise_summary = {}
    if localise_groups is not None:
        lp = os.path.join(output_directory, "localisation.sage.tsv")
        cols = [np.concatenate([p[j] for p in localise_parts]) if localise_parts else np.zeros(0) for j in range(9)]
        rows = output.localisation_rows(host, flat, list(order), psm_ids, *cols)
        output.write_localisation(lp, rows)
        paths.append(lp)
        localise_summary = {"localisation_rows": len(rows), "localisation_ms": localise_ms}
        log(f"- localisation:   {int(localise_ms):8d} ms ({len(rows)} PSMs with positional isomers)")
    if tmt_parts:  # runner.rs:638-641: only when some spectrum was quantified
        tp = os.path.join(output_directory, "tmt.tsv")
        output.write_tmt_native(tp, isobaric.headers(), filenames, np.concatenate([np.full(len(p[1]), p[0], np.uint32) for p in tmt_parts]),
                                [s for p in tmt_parts for s in p[1]], np.concatenate([p[2] for p in tmt_parts]),
                                np.concatenate([p[3] for p in tmt_parts]))
        paths.append(tp)
    if lfq_result is not None:  # runner.rs:643-647
        lp = os.path.join(output_directory, "lfq.tsv")
        output.write_lfq_native(lp, host, lfq_result, filenames)
        paths.append(lp)
    protein_lfq_summary = {}
    if lfq_result is not None and protein_lfq_on:  # MaxLFQ over lfq.tsv's rows, one protein (group) per peptide
        t0 = time.time()
        used, ids, names = output.protein_lfq_assignment(host, lfq_result, flat, groups, protein_lfq_st["precursor_q_value"])
        rolled = protein_lfq(lfq_result.areas[used.astype(np.int64)].reshape(len(used), len(filenames)), ids, len(names),
                             protein_lfq_st["min_ratio_count"], device=device)
        pp = os.path.join(output_directory, "protein_lfq.tsv")
        n_written = output.write_protein_lfq_native(pp, names, rolled, filenames)
        paths.append(pp)
        protein_lfq_ms = (time.time() - t0) * 1000.0
        log(f"- protein roll-up (MaxLFQ): {int(protein_lfq_ms):8d} ms ({n_written} proteins from {len(used)} precursors)")
        protein_lfq_summary = {"protein_lfq_rows": n_written, "protein_lfq_ms": protein_lfq_ms,
                               "protein_lfq_device_ms": rolled.stage_ms["device_ms"]}
    purity_summary = {}
    if purity_on:  # one query per reported PSM, in results.sage.tsv's order, on the first device
        t0 = time.time()
        o = np.array(list(order), dtype=np.int64)
        cols = [np.concatenate([p[j] for p in purity_parts])[o] if purity_parts else np.zeros(0, np.float32) for j in range(4)]
        fid, charge = flat["file_id"][o], flat["charge"][o].astype(np.uint8)
        ms1_index = assign_ms1(ms1_batches, fid, cols[3])
        pur = precursor_purity(ms1_batches, ms1_index, cols[0], charge, cols[1], cols[2], purity_st["ppm_tolerance"],
                               purity_st["max_isotope"], purity_st["default_isolation"], device=device)
        ms1_ids = [s for b in ms1_batches for s in b.ids]
        missing = np.isnan(cols[1]) | np.isnan(cols[2])
        used_lo = np.where(missing, np.float32(purity_st["default_isolation"][0]), cols[1]).astype(np.float32)
        used_hi = np.where(missing, np.float32(purity_st["default_isolation"][1]), cols[2]).astype(np.float32)
        up = os.path.join(output_directory, "purity.sage.tsv")
        output.write_purity_native(up, [psm_ids[i] for i in o], filenames, fid, [spec_ids[i] for i in o], charge,
                                   ["" if int(k) == NO_MS1 else ms1_ids[int(k)] for k in ms1_index], used_lo, used_hi, pur)
        paths.append(up)
        purity_ms = (time.time() - t0) * 1000.0
        log(f"- precursor purity: {int(purity_ms):8d} ms ({len(o)} PSMs, {pur.stage_ms['device_ms']:.1f} ms on the device)")
        purity_summary = {"purity_rows": len(o), "purity_ms": purity_ms}
    tmt_rollup_summary = {}
    if tmt_rollup_on and tmt_parts and isobaric.headers():  # tmt.tsv's rows joined to the PSMs, filtered, rolled up plex by plex
        t0 = time.time()
        st = tmt_rollup_st
        row_file = np.concatenate([np.full(len(p[1]), p[0], np.uint32) for p in tmt_parts])
        row_ids = [s for p in tmt_parts for s in p[1]]
        reporter = np.concatenate([p[3] for p in tmt_parts]).reshape(len(row_ids), -1)
        purity_of = None
        if st["min_purity"] is not None:  # (purity's block above: its results are in results.sage.tsv's order)
            purity_of = np.full(len(flat), -1.0, np.float32)
            purity_of[o] = pur.purity
        spectrum_q = post.spectrum_q if post is not None else np.zeros(0, np.float32)
        ids, names, peptide_of = output.tmt_rollup_assignment(host, flat, spec_ids, spectrum_q, row_file, row_ids, groups, purity_of,
                                                              st["psm_q_value"], st["min_purity"], st["by"])
        plex_of_file = st["plex_of_file"] if st["plex_of_file"] is not None else [0] * len(filenames)
        row_plex = np.array(plex_of_file, np.int64)[row_file.astype(np.int64)]
        plexes, rollup_device_ms = [], 0.0
        for plex in sorted(set(row_plex.tolist())):
            at = np.flatnonzero(row_plex == plex)
            rolled = tmt_rollup(reporter[at], ids[at], len(names), st["min_channels"], st["normalise"], st["summary"], device=device)
            rollup_device_ms += rolled.stage_ms["device_ms"]
            plexes.append((plex, rolled, ids[at], peptide_of[at], reporter[at]))
        table = output.tmt_rollup_table(plexes, st["min_channels"])
        rp = os.path.join(output_directory, "tmt_proteins.tsv" if st["by"] == "protein" else "tmt_peptides.tsv")
        n_written = output.write_tmt_rollup_native(rp, "proteins" if st["by"] == "protein" else "peptide", isobaric.headers(), names, table)
        paths.append(rp)
        tmt_rollup_ms = (time.time() - t0) * 1000.0
        log(f"- TMT roll-up ({st['summary']}, {st['normalise']}): {int(tmt_rollup_ms):8d} ms ({n_written} rows of {len(names)} "
            f"{'proteins' if st['by'] == 'protein' else 'peptides'} from {int((ids != output.NO_GROUP).sum())} of {len(ids)} spectra, "
            f"{len(plexes)} plex{'es' if len(plexes) != 1 else ''})")
        tmt_rollup_summary = {"tmt_rollup_rows": n_written, "tmt_rollup_ms": tmt_rollup_ms, "tmt_rollup_device_ms": rollup_device_ms}
    if write_pin:  # runner.rs:655-660
        pp = os.path.join(output_directory, "results.sage.pin")
        output.write_results_native(pp, "pin", host, flat, list(order), psm_ids, filenames, spec_ids, [rtp, post])
        paths.append(pp)
    stage_totals["write_ms"] = (time.time() - t_write) * 1e3
    log(f"- writing: {int(stage_totals['write_ms']):8d} ms")
    if lfq_summary:
        stage_totals["lfq_ms"] = lfq_summary["lfq_ms"]
    tmt_summary = {}
    if isobaric is not None:
        log(f"- TMT quantification: {int(tmt_ms):8d} ms")
        tmt_summary = {"tmt_rows": sum(len(p[1]) for p in tmt_parts), "tmt_ms": tmt_ms}
    stage_totals["total_after_index_ms"] = (time.time() - t_run) * 1e3
    summary = {"version": "sage-hip 0.1 (search-and-score path of sage 0.15.0-beta.2)", "psms": len(flat),
               "spectra_searched": n_searched, "search_ms": search_ms, "stages": stage_totals, "output_paths": paths, **rescore_summary,
               **lfq_summary, **tmt_summary, **isomer_summary, **localise_summary, **protein_lfq_summary, **purity_summary, **tmt_rollup_summary}
    with open(os.path.join(output_directory, "results.json"), "w") as fh:
        json.dump(dict(cfg, output_paths=paths, summary=summary), fh, indent=2, default=str)
    return summary


def main(argv=None):
    ap = argparse.ArgumentParser(prog="sage_amd.cli", description="GPU search-and-score path of Sage (JSON-config CLI)")
    ap.add_argument("parameters", help="path to configuration parameters (JSON file)")
    ap.add_argument("mzml_paths", nargs="*", help="paths to mzML files to process. Overrides mzML files listed in the configuration file.")
    ap.add_argument("-f", "--fasta", help="path to FASTA database. Overrides the FASTA file specified in the configuration file.")
    ap.add_argument("-o", "--output_directory", help="where to place output files. Overrides the directory specified in the configuration file.")
    ap.add_argument("--annotate-matches", action="store_true", help="write matched fragments output file")
    ap.add_argument("--write-pin", action="store_true", help="write percolator-compatible `.pin` output files")
    # accepted for command-line compatibility with sage (sage-cli/src/main.rs:55-97)
    ap.add_argument("--batch-size", type=int, help="number of files sage loads and searches in parallel; files are searched one "
                                                   "after the other here (every file is one resident GPU batch)")
    ap.add_argument("--parquet", action="store_true", help="not supported by this path (tsv only)")
    ap.add_argument("--write-report", action="store_true", help="not supported by this path")
    ap.add_argument("--disable-telemetry-i-dont-want-to-improve-sage", action="store_true", dest="disable_telemetry",
                    help="accepted; this implementation never sends telemetry")
    ap.add_argument("--stack-size", type=int, help="accepted; no effect")
    ap.add_argument("--device", type=int, default=0, help="the HIP device that searches (default 0)")
    ap.add_argument("--devices", help="search on several devices at once: all | 0-7 | 0,2,3 — every file's spectra are sharded "
                                      "over them, the index is replicated (sage uses every core of the machine; this is the same)")
    ap.add_argument("--host-preprocess", action="store_true", help="run SpectrumProcessor::process on the host instead of the device")
    args = ap.parse_args(argv)
    if args.parquet or args.write_report:
        raise SystemExit("sage_amd.cli: --parquet / --write-report are outside the search-and-score path (tsv / pin output only)")
    if args.batch_size is not None and args.batch_size < 1:
        raise SystemExit("error: invalid value for '--batch-size': must be >= 1")
    cfg = json.load(open(args.parameters))
    if args.fasta:
        cfg.setdefault("database", {})["fasta"] = args.fasta
    if args.annotate_matches:
        cfg["annotate_matches"] = True
    mzml = args.mzml_paths or cfg.get("mzml_paths")
    if not mzml:
        raise SystemExit("'mzml_paths' must be provided!")
    out = args.output_directory or cfg.get("output_directory") or os.getcwd()
    summary = run(cfg, mzml, out, args.device, host_preprocess=args.host_preprocess,
                  write_pin=args.write_pin or bool(cfg.get("write_pin", False)),
                  devices=parse_devices(args.devices, device_count()))
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
