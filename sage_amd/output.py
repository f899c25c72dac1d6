"""results.sage.tsv / matched_fragments.sage.tsv writers (host side).

Column order and number formatting follow the reference byte for byte where the hot path owns the value:
sage-cli/src/runner.rs:687-780 (serialize_feature), :782-828 (serialize_fragments), :830-935 (headers).  Integers are
written with `itoa`, floats with `ryu` (shortest digits that round-trip, Rust `ryu::Buffer::format`), reproduced by
`ryu_f32` / `ryu_f64` below.  sage_discriminant_score, posterior_error, spectrum_q, peptide_q and protein_q come from the
device rescoring (sage_hip_rescore), aligned_rt / predicted_rt / delta_rt_model / predicted_mobility / delta_mobility from
sage_hip_predict_rt when `predict_rt` is on (the default, input.rs:372), protein_groups / num_protein_groups / protein_group_q
from sage_hip_protein_groups; where a stage did not run, the defaults Feature gets in build_features (scoring.rs:576-592):
predicted_rt 0.0, aligned_rt = rt, delta_rt_model / delta_ims_model 0.999, no protein groups (an empty field, 0),
protein_group_q 1.0.  `results.sage.pin` follows runner.rs:938-1135.
"""
import ctypes
import re
from typing import List, Optional, Sequence

import numpy as np

HEADERS = ["psm_id", "peptide", "proteins", "protein_groups", "num_proteins", "num_protein_groups", "filename", "scannr",
           "rank", "label", "expmass", "calcmass", "charge", "peptide_len", "missed_cleavages", "semi_enzymatic",
           "isotope_error", "precursor_ppm", "fragment_ppm", "hyperscore", "delta_next", "delta_best", "rt", "aligned_rt",
           "predicted_rt", "delta_rt_model", "ion_mobility", "predicted_mobility", "delta_mobility", "matched_peaks",
           "longest_b", "longest_y", "longest_y_pct", "matched_intensity_pct", "scored_candidates", "poisson",
           "sage_discriminant_score", "posterior_error", "spectrum_q", "peptide_q", "protein_q", "protein_group_q",
           "ms2_intensity"]
FRAGMENT_HEADERS = ["psm_id", "fragment_type", "fragment_ordinals", "fragment_charge", "fragment_mz_calculated",
                    "fragment_mz_experimental", "fragment_intensity"]
ION_NAMES = "abcxyz"


def _ryu(x, f32: bool) -> str:
    """ryu::Buffer::format: shortest round-trip digits, laid out as ryu's pretty printer does (ryu/src/pretty/mod.rs:
    plain decimals while the decimal point stays within 16 (f64) / 13 (f32) digits and the value is >= 1e-5 (f64) /
    1e-6 (f32); otherwise d.ddde[-]x)."""
    x = np.float32(x) if f32 else np.float64(x)
    if np.isnan(x):
        return "NaN"
    if np.isinf(x):
        return "inf" if x > 0 else "-inf"
    if x == 0:
        return "-0.0" if np.signbit(x) else "0.0"
    sci = np.format_float_scientific(x, unique=True, trim="-", exp_digits=1)  # e.g. '1.2345e+3', '-5e-7'
    sign = "-" if sci[0] == "-" else ""
    mant, exp = sci.lstrip("-").split("e")
    digits = mant.replace(".", "")
    e10 = int(exp)
    length = len(digits)
    kk = e10 + 1            # 10^(kk-1) <= |x| < 10^kk
    k = kk - length         # x = digits * 10^k
    hi = 13 if f32 else 16
    lo = -6 if f32 else -5
    if 0 <= k and kk <= hi:
        return sign + digits + "0" * k + ".0"
    if 0 < kk <= hi:
        return sign + digits[:kk] + "." + digits[kk:]
    if lo < kk <= 0:
        return sign + "0." + "0" * (-kk) + digits
    if length == 1:
        return sign + digits + "e" + str(kk - 1)
    return sign + digits[0] + "." + digits[1:] + "e" + str(kk - 1)


def ryu_f32(x) -> str:
    return _ryu(x, True)


def ryu_f64(x) -> str:
    return _ryu(x, False)


DEFAULT_POST = dict(discriminant_score=0.0, posterior_error=1.0, spectrum_q=1.0, peptide_q=1.0, protein_q=1.0)


def feature_row(psm_id: int, f, db, filename: str, scannr: str, post: Optional[dict] = None, protein_groups: Optional[str] = None,
                num_protein_groups: int = 0, protein_group_q=1.0) -> List[str]:
    """serialize_feature (runner.rs:687-780) for one SageFeature record `f` (numpy void of FEATURE_DTYPE); `post` = the
    rescoring outputs of this PSM (defaults of scoring.rs:576-592 when the rescoring did not run); protein_groups /
    num_protein_groups / protein_group_q = the protein-group stage's (None, 0, 1.0 when it did not run)."""
    post = dict(DEFAULT_POST, **(post or {}))
    pep = int(f["peptide_idx"])
    num_proteins, semi = db.peptide_info(pep)
    rt = f["rt"]
    aligned_rt = post.get("aligned_rt", rt)  # Feature defaults without the predict_rt block: scoring.rs:576-592
    predicted_rt, delta_rt = post.get("predicted_rt", 0.0), post.get("delta_rt_model", 0.999)
    predicted_ims, delta_ims = post.get("predicted_ims", 0.0), post.get("delta_ims_model", 0.999)
    return [
        str(psm_id), db.peptide_string(pep), db.peptide_proteins(pep), protein_groups or "", str(num_proteins), str(int(num_protein_groups)),
        filename, scannr,
        str(int(f["rank"])), str(int(f["label"])), ryu_f32(f["expmass"]), ryu_f32(f["calcmass"]), str(int(f["charge"])),
        str(int(f["peptide_len"])), str(int(f["missed_cleavages"])), str(semi), ryu_f32(f["isotope_error"]),
        ryu_f32(f["delta_mass"]), ryu_f32(f["average_ppm"]), ryu_f64(f["hyperscore"]), ryu_f64(f["delta_next"]),
        ryu_f64(f["delta_best"]), ryu_f32(rt), ryu_f32(aligned_rt), ryu_f32(predicted_rt), ryu_f32(delta_rt), ryu_f32(f["ims"]),
        ryu_f32(predicted_ims), ryu_f32(delta_ims), str(int(f["matched_peaks"])), str(int(f["longest_b"])), str(int(f["longest_y"])),
        ryu_f32(f["longest_y_pct"]), ryu_f32(f["matched_intensity_pct"]), str(int(f["scored_candidates"])),
        ryu_f64(f["poisson"]), ryu_f32(post["discriminant_score"]), ryu_f32(post["posterior_error"]),
        ryu_f32(post["spectrum_q"]), ryu_f32(post["peptide_q"]), ryu_f32(post["protein_q"]), ryu_f32(protein_group_q),
        ryu_f32(f["ms2_intensity"]),
    ]


def csv_field(s: str) -> str:
    """a field as the csv crate writes it with QuoteStyle::Necessary (runner.rs:837-839, 907-909): quoted, inner quotes
    doubled, when it contains a quote, tab, CR or LF"""
    if any(c in s for c in '"\t\r\n'):
        return '"' + s.replace('"', '""') + '"'
    return s


def _record(fields) -> str:
    return "\t".join(csv_field(f) for f in fields)


def write_features(path: str, rows: Sequence[List[str]]) -> None:
    """write_features (runner.rs:830-905): tab-separated, header first."""
    with open(path, "w", newline="") as fh:
        fh.write(_record(HEADERS) + "\n")
        for r in rows:
            fh.write(_record(r) + "\n")


def fragment_rows(psm_id: int, lo: int, hi: int, arr) -> List[List[str]]:
    """serialize_fragments (runner.rs:782-828) for entries [lo, hi) of the flat Fragments arrays."""
    return [[str(psm_id), ION_NAMES[int(arr["kinds"][j])], str(int(arr["fragment_ordinals"][j])), str(int(arr["charges"][j])),
             ryu_f32(arr["mz_calculated"][j]), ryu_f32(arr["mz_experimental"][j]), ryu_f32(arr["intensities"][j])]
            for j in range(lo, hi)]


def write_fragments(path: str, rows: Sequence[List[str]]) -> None:
    with open(path, "w", newline="") as fh:
        fh.write(_record(FRAGMENT_HEADERS) + "\n")
        for r in rows:
            fh.write(_record(r) + "\n")


ISOMER_HEADERS = ["psm_id", "peptide", "isomers", "best_isomer", "isomer_hyperscore", "isomer_matched_peaks", "delta_isomer"]


def isomer_rows(db, features, order, psm_ids, n_isomers, best_pep, best_hyperscore, best_matched) -> List[List[str]]:
    """isomers.sage.tsv (an addition over the reference): one row per PSM whose peptide has positional isomers, in the row order of
    results.sage.tsv.  The arrays are indexed like `features`; delta_isomer = hyperscore - isomer_hyperscore in f64."""
    rows = []
    for i in order:
        if int(n_isomers[i]) == 0:
            continue
        h, hi = np.float64(features[i]["hyperscore"]), np.float64(best_hyperscore[i])
        rows.append([str(psm_ids[i]), db.peptide_string(int(features[i]["peptide_idx"])), str(int(n_isomers[i])),
                     db.peptide_string(int(best_pep[i])), ryu_f64(hi), str(int(best_matched[i])), ryu_f64(h - hi)])
    return rows


def write_isomers(path: str, rows: Sequence[List[str]]) -> None:
    with open(path, "w", newline="") as fh:
        fh.write(_record(ISOMER_HEADERS) + "\n")
        for r in rows:
            fh.write(_record(r) + "\n")


LOCALISATION_HEADERS = ["psm_id", "peptide", "placements", "best_placement", "peptide_score", "second_placement",
                        "second_peptide_score", "site_determining_ions", "depth", "ascore", "reported_is_best"]


def localisation_rows(db, features, order, psm_ids, placements, best_pep, best_score, second_pep, second_score, n_site_items, depth,
                      ascore, reported_is_best) -> List[List[str]]:
    """localisation.sage.tsv (an addition over the reference): one row per PSM whose peptide has positional isomers,
    in the row order of results.sage.tsv.  The arrays are indexed like `features`; placements counts the reported peptide."""
    rows = []
    for i in order:
        if int(placements[i]) == 0:
            continue
        rows.append([str(psm_ids[i]), db.peptide_string(int(features[i]["peptide_idx"])), str(int(placements[i])),
                     db.peptide_string(int(best_pep[i])), ryu_f64(np.float64(best_score[i])), db.peptide_string(int(second_pep[i])),
                     ryu_f64(np.float64(second_score[i])), str(int(n_site_items[i])), str(int(depth[i])), ryu_f64(np.float64(ascore[i])),
                     "true" if reported_is_best[i] else "false"])
    return rows


def write_localisation(path: str, rows: Sequence[List[str]]) -> None:
    with open(path, "w", newline="") as fh:
        fh.write(_record(LOCALISATION_HEADERS) + "\n")
        for r in rows:
            fh.write(_record(r) + "\n")


PIN_HEADERS = ["SpecId", "Label", "ScanNr", "ExpMass", "CalcMass", "FileName", "retentiontime", "ion_mobility", "rank", "z=2",
               "z=3", "z=4", "z=5", "z=6", "z=other", "peptide_len", "missed_cleavages", "semi_enzymatic", "isotope_error",
               "ln(precursor_ppm)", "fragment_ppm", "ln(hyperscore)", "ln(delta_next)", "ln(delta_best)", "aligned_rt",
               "predicted_rt", "sqrt(delta_rt_model)", "predicted_mobility", "sqrt(delta_mobility)", "matched_peaks", "longest_b",
               "longest_y", "longest_y_pct", "ln(matched_intensity_pct)", "scored_candidates", "ln(-poisson)", "posterior_error",
               "Peptide", "Proteins"]
_SCAN_RE = re.compile(r"scan=(\d+)")
_libm = ctypes.CDLL("libm.so.6")
_libm.log1pf.restype = ctypes.c_float
_libm.log1pf.argtypes = [ctypes.c_float]
_libm.log1p.restype = ctypes.c_double
_libm.log1p.argtypes = [ctypes.c_double]


def _ln1p_f32(x) -> np.float32:  # f32::ln_1p == libm log1pf
    return np.float32(_libm.log1pf(float(np.float32(x))))


def _ln1p_f64(x) -> np.float64:
    return np.float64(_libm.log1p(float(x)))


def pin_row(psm_id: int, f, db, filename: str, spec_id: str, post: Optional[dict] = None) -> List[str]:
    """serialize_pin (runner.rs:938-1084): percolator input, log / sqrt transformed feature columns."""
    post = dict(DEFAULT_POST, **(post or {}))
    pep = int(f["peptide_idx"])
    _, semi = db.peptide_info(pep)
    caps = _SCAN_RE.findall(spec_id)
    scannr = caps[-1] if caps else spec_id
    z = int(f["charge"])
    rt = f["rt"]
    aligned_rt = post.get("aligned_rt", rt)
    predicted_rt, predicted_ims = post.get("predicted_rt", 0.0), post.get("predicted_ims", 0.0)
    d = np.float32(post.get("delta_rt_model", 0.999))
    delta_rt = np.float32(0.001) if d < np.float32(0.001) else (np.float32(1.0) if d > np.float32(1.0) else d)  # .clamp(0.001, 1.0)
    delta_ims = post.get("delta_ims_model", 0.999)
    return [
        str(psm_id), str(int(f["label"])), scannr, ryu_f32(f["expmass"]), ryu_f32(f["calcmass"]), filename, ryu_f32(rt),
        ryu_f32(f["ims"]), str(int(f["rank"])), str(int(z == 2)), str(int(z == 3)), str(int(z == 4)), str(int(z == 5)),
        str(int(z == 6)), str(z if (z < 2 or z > 6) else 0), str(int(f["peptide_len"])), str(int(f["missed_cleavages"])),
        str(semi), ryu_f32(f["isotope_error"]), ryu_f32(_ln1p_f32(np.abs(np.float32(f["delta_mass"])))),
        ryu_f32(f["average_ppm"]), ryu_f64(_ln1p_f64(f["hyperscore"])), ryu_f64(_ln1p_f64(f["delta_next"])),
        ryu_f64(_ln1p_f64(f["delta_best"])), ryu_f32(aligned_rt), ryu_f32(predicted_rt), ryu_f32(np.sqrt(delta_rt, dtype=np.float32)),
        ryu_f32(predicted_ims), ryu_f32(delta_ims), str(int(f["matched_peaks"])), str(int(f["longest_b"])), str(int(f["longest_y"])),
        ryu_f32(f["longest_y_pct"]), ryu_f32(_ln1p_f32(f["matched_intensity_pct"])), str(int(f["scored_candidates"])),
        ryu_f64(_ln1p_f64(-np.float64(f["poisson"]))), ryu_f32(post["posterior_error"]), db.peptide_string(pep),
        db.peptide_proteins(pep),
    ]


def write_pin(path: str, rows: Sequence[List[str]]) -> None:
    """write_pin (runner.rs:1086-1135)."""
    with open(path, "w", newline="") as fh:
        fh.write(_record(PIN_HEADERS) + "\n")
        for r in rows:
            fh.write(_record(r) + "\n")


def write_results_native(path: str, fmt: str, db, features, order, psm_ids, filenames, spec_ids, post=None, groups=None) -> None:
    """results.sage.tsv (fmt "tsv") / results.sage.pin (fmt "pin") through the C++ writer (sage_hip_write_results): the same
    bytes as feature_row / pin_row + write_features / write_pin, without a Python loop per PSM.  `post`: RescoreResult-like
    and / or RtPrediction-like objects (attributes named like SagePostColumns), or None.  `groups`: a ProteinGroupResult-like
    object (strings, string_id, num_protein_groups, protein_group_q) — then through sage_hip_write_results_grouped."""
    import ctypes as C

    from . import _lib as L

    f = np.ascontiguousarray(features, dtype=L.FEATURE_DTYPE).reshape(-1)
    n = len(f)
    order_a = None if order is None else np.ascontiguousarray(order, dtype=np.uint64)
    ids = np.ascontiguousarray(psm_ids, dtype=np.uint64)
    assert len(ids) == n and len(spec_ids) == n and (order_a is None or len(order_a) == n)
    names = (C.c_char_p * max(len(filenames), 1))(*[s.encode() for s in filenames])
    specs = (C.c_char_p * max(n, 1))(*[s.encode() for s in spec_ids])
    cols = L.SagePostColumns()
    keep = []
    for source in (post if isinstance(post, (list, tuple)) else [post]):
        for k, _ in L.SagePostColumns._fields_:
            a = getattr(source, k, None) if source is not None else None
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float32)
                assert len(a) == n
                keep.append(a)
                setattr(cols, k, L.as_ptr(a, C.c_float))
    args = (path.encode(), {"tsv": 0, "pin": 1}[fmt], db._h, f.ctypes.data, n, None if order_a is None else L.as_ptr(order_a, C.c_uint64),
            L.as_ptr(ids, C.c_uint64), names, len(filenames), specs, C.byref(cols))
    if groups is None:
        L.check(L.load().sage_hip_write_results(*args))
        return
    sid = np.ascontiguousarray(groups.string_id, dtype=np.uint32)
    num = np.ascontiguousarray(groups.num_protein_groups, dtype=np.uint32)
    gq = np.ascontiguousarray(groups.protein_group_q, dtype=np.float32)
    assert len(sid) == n and len(num) == n and len(gq) == n
    table = (C.c_char_p * max(len(groups.strings), 1))(*[s.encode() for s in groups.strings])
    gcols = L.SageGroupColumns(table, len(groups.strings), L.as_ptr(sid, C.c_uint32), L.as_ptr(num, C.c_uint32), L.as_ptr(gq, C.c_float))
    L.check(L.load().sage_hip_write_results_grouped(*args, C.byref(gcols)))


LFQ_HEADERS = ["peptide", "charge", "proteins", "q_value", "score", "spectral_angle"]


def lfq_rows(db, result, rows) -> List[List[str]]:
    """write_lfq (runner.rs:1182-1235) for the grids `rows` of an LfqResult: charge -1 when charge states are combined,
    q_value f32, score / spectral_angle / areas f64."""
    out = []
    for i in rows:
        i = int(i)
        pep = int(result.peptide_idx[i])
        z = int(result.charge[i])
        out.append([db.peptide_string(pep), str(z if z else -1), db.peptide_proteins(pep), ryu_f32(result.q_value[i]),
                    ryu_f64(result.score[i]), ryu_f64(result.spectral_angle[i])] + [ryu_f64(a) for a in result.areas[i]])
    return out


def write_lfq(path: str, filenames: Sequence[str], rows: Sequence[List[str]]) -> None:
    with open(path, "w", newline="") as fh:
        fh.write(_record(LFQ_HEADERS + list(filenames)) + "\n")
        for r in rows:
            fh.write(_record(r) + "\n")


def write_lfq_native(path: str, db, result, filenames: Sequence[str], rows=None) -> None:
    """lfq.tsv through the C++ writer (sage_hip_write_lfq): the bytes of lfq_rows + write_lfq.  rows: grid indices, default
    the target grids with a peak in grid order (ascending peptide index, then charge)."""
    import ctypes as C

    from . import _lib as L
    rows = np.ascontiguousarray(result.target_rows() if rows is None else rows, dtype=np.uint64)
    keep = []
    cout = result.to_c(keep)
    names = (C.c_char_p * max(len(filenames), 1))(*[s.encode() for s in filenames])
    L.check(L.load().sage_hip_write_lfq(path.encode(), db._h, C.byref(cout), L.as_ptr(rows, C.c_uint64), len(rows), names,
                                        len(filenames)))


PROTEIN_LFQ_HEADERS = ["proteins", "n_precursors", "n_components"]


def protein_lfq_assignment(db, lfq_result, features=None, groups=None, precursor_q_value: float = 0.05):
    """The input of api.protein_lfq from a run's LfqResult: (grid rows used, protein id of each, protein names by
    id).  Rows: lfq.tsv's (LfqResult.target_rows()) with q_value <= precursor_q_value whose peptide belongs to one protein only —
    with `groups` (a ProteinGroupResult over `features`, the run's PSMs) the peptide's protein_groups string where its
    num_protein_groups == 1, else the peptide's `proteins` string where its num_proteins == 1.  Shared peptides are left out.
    Ids by first appearance in grid order."""
    by_peptide = {}
    if groups is not None:
        for i, pep in enumerate(np.asarray(features["peptide_idx"]).tolist()):
            if pep not in by_peptide:
                by_peptide[pep] = (groups.protein_groups(i), int(groups.num_protein_groups[i]))
    rows, ids, names, id_of = [], [], [], {}
    for i in lfq_result.target_rows().tolist():
        if not lfq_result.q_value[i] <= np.float32(precursor_q_value):
            continue
        pep = int(lfq_result.peptide_idx[i])
        if groups is not None:
            name, count = by_peptide.get(pep, ("", 0))
        else:
            name, count = db.peptide_proteins(pep), db.peptide_info(pep)[0]
        if count != 1:
            continue
        if name not in id_of:
            id_of[name] = len(names)
            names.append(name)
        rows.append(i)
        ids.append(id_of[name])
    return np.array(rows, np.uint64), np.array(ids, np.uint32), names


def protein_lfq_rows(names: Sequence[str], result, rows=None) -> List[List[str]]:
    """protein_lfq.tsv's rows for a ProteinLfqResult-like object (n_rows_used, n_components, intensity): one per protein id of
    `rows` (default: every protein with at least one used row, in id order); the intensities as ryu f64, 0.0 = not quantified."""
    rows = np.flatnonzero(np.asarray(result.n_rows_used) > 0) if rows is None else rows
    return [[names[int(p)], str(int(result.n_rows_used[int(p)])), str(int(result.n_components[int(p)]))] +
            [ryu_f64(np.float64(x)) for x in result.intensity[int(p)]] for p in rows]


def write_protein_lfq(path: str, filenames: Sequence[str], rows: Sequence[List[str]]) -> None:
    with open(path, "w", newline="") as fh:
        fh.write(_record(PROTEIN_LFQ_HEADERS + list(filenames)) + "\n")
        for r in rows:
            fh.write(_record(r) + "\n")


def write_protein_lfq_native(path: str, names: Sequence[str], result, filenames: Sequence[str], rows=None) -> int:
    """protein_lfq.tsv through the C++ writer (sage_hip_write_protein_lfq): the bytes of protein_lfq_rows + write_protein_lfq.
    Returns the number of rows written."""
    import ctypes as C

    from . import _lib as L
    rows = np.ascontiguousarray(np.flatnonzero(np.asarray(result.n_rows_used) > 0) if rows is None else rows, dtype=np.uint32)
    keep = []
    cout = result.to_c(keep)
    table = (C.c_char_p * max(len(names), 1))(*[s.encode() for s in names])
    files = (C.c_char_p * max(len(filenames), 1))(*[s.encode() for s in filenames])
    L.check(L.load().sage_hip_write_protein_lfq(path.encode(), table, len(names), L.as_ptr(rows, C.c_uint32), len(rows), C.byref(cout),
                                                files, len(filenames)))
    return len(rows)


TMT_ROLLUP_HEADERS = ["plex", "n_psms", "n_peptides"]
NO_GROUP = 0xFFFFFFFF  # group_of_row of a tmt.tsv row that takes no part in the roll-up


def tmt_rollup_assignment(db, features, spec_ids, spectrum_q, tmt_file_id, tmt_spec_ids, groups=None, purity=None,
                          psm_q_value: float = 0.01, min_purity=None, by: str = "protein"):
    """The input of api.tmt_rollup from a run's PSMs and its tmt.tsv rows: (group id of every tmt.tsv row, names by
    id, peptide index of every row or -1).  features / spec_ids / spectrum_q / purity: the run's PSMs (purity: f32 per PSM or None);
    tmt_file_id / tmt_spec_ids: tmt.tsv's rows in its own order (the scannr is the MS2's id: at another quant level the MS3's
    precursor_ref).  A row takes the group of the first rank-1 target PSM of its (file, scannr), when that PSM has spectrum_q <=
    psm_q_value (f32), a peptide of one protein only — with `groups` (a ProteinGroupResult over the PSMs) one protein group, by the
    rule of protein_lfq_assignment — and, with min_purity, a purity >= min_purity (f32; -1.0 fails).  Any other row: NO_GROUP.
    by: "protein" (the proteins / protein_groups string names the group) or "peptide" (the peptide's modified sequence).  Ids by
    first appearance in tmt.tsv's order."""
    assert by in ("protein", "peptide")
    first = {}
    fid, rank, label = np.asarray(features["file_id"]), np.asarray(features["rank"]), np.asarray(features["label"])
    for i in range(len(fid)):
        if int(rank[i]) == 1 and int(label[i]) == 1:
            first.setdefault((int(fid[i]), spec_ids[i]), i)
    ids, peptide, names, id_of = [], [], [], {}
    for f, s in zip(np.asarray(tmt_file_id).tolist(), tmt_spec_ids):
        i = first.get((int(f), s))
        ids.append(NO_GROUP)
        peptide.append(-1)
        if i is None or not np.float32(spectrum_q[i]) <= np.float32(psm_q_value):
            continue
        if min_purity is not None and not np.float32(purity[i]) >= np.float32(min_purity):
            continue
        pep = int(features["peptide_idx"][i])
        if groups is not None:
            name, count = groups.protein_groups(i), int(groups.num_protein_groups[i])
        else:
            name, count = db.peptide_proteins(pep), db.peptide_info(pep)[0]
        if count != 1:
            continue
        if by == "peptide":
            name = db.peptide_string(pep)
        if name not in id_of:
            id_of[name] = len(names)
            names.append(name)
        ids[-1], peptide[-1] = id_of[name], pep
    return np.array(ids, np.uint32), names, np.array(peptide, np.int64)


def tmt_rollup_table(plexes, min_present: int = 1):
    """The rows of tmt_proteins.tsv from the plexes' results: plexes = [(plex id, TmtRollupResult-like, group_of_row, peptide_of_row,
    intensity)] over the rows of each plex.  One row per (group, plex) with at least one used row, ascending group id, then plex:
    (group ids, plex ids, n_psms, n_peptides, abundance [rows, n_labels]).  n_peptides: the distinct peptides of the used rows (those
    with at least max(min_present, 1) present cells)."""
    out = []
    for plex, result, group_of_row, peptide_of_row, intensity in plexes:
        x = np.asarray(intensity, dtype=np.float32).reshape(len(group_of_row), -1).astype(np.float64)
        n_present = ((x > 0) & (x < np.inf)).sum(axis=1)
        peptides = {}
        for g, pep, c in zip(np.asarray(group_of_row).tolist(), np.asarray(peptide_of_row).tolist(), n_present.tolist()):
            if g != NO_GROUP and c >= max(int(min_present), 1):
                peptides.setdefault(g, set()).add(pep)
        for g in np.flatnonzero(np.asarray(result.n_rows_used) > 0).tolist():
            assert len(peptides.get(g, ())) > 0
            out.append((g, int(plex), int(result.n_rows_used[g]), len(peptides[g]), np.asarray(result.abundance[g], np.float64)))
    out.sort(key=lambda r: (r[0], r[1]))
    n_labels = len(out[0][4]) if out else 0
    return (np.array([r[0] for r in out], np.uint32), np.array([r[1] for r in out], np.uint32), np.array([r[2] for r in out], np.uint32),
            np.array([r[3] for r in out], np.uint32), np.array([r[4] for r in out], np.float64).reshape(len(out), n_labels))


def tmt_rollup_rows(names: Sequence[str], table) -> List[List[str]]:
    """tmt_proteins.tsv's rows for a tmt_rollup_table: the abundances as ryu f64, 0.0 = not quantified."""
    gid, plex, n_psms, n_peptides, abundance = table
    return [[names[int(g)], str(int(p)), str(int(a)), str(int(b))] + [ryu_f64(np.float64(x)) for x in row]
            for g, p, a, b, row in zip(gid, plex, n_psms, n_peptides, abundance)]


def write_tmt_rollup(path: str, first_header: str, headers: Sequence[str], rows: Sequence[List[str]]) -> None:
    with open(path, "w", newline="") as fh:
        fh.write(_record([first_header] + TMT_ROLLUP_HEADERS + list(headers)) + "\n")
        for r in rows:
            fh.write(_record(r) + "\n")


def write_tmt_rollup_native(path: str, first_header: str, headers: Sequence[str], names: Sequence[str], table) -> int:
    """tmt_proteins.tsv through the C++ writer (sage_hip_write_tmt_rollup): the bytes of tmt_rollup_rows + write_tmt_rollup.
    Returns the number of rows written."""
    import ctypes as C

    from . import _lib as L
    gid, plex, n_psms, n_peptides, abundance = table
    plex, n_psms, n_peptides = (np.ascontiguousarray(a, dtype=np.uint32) for a in (plex, n_psms, n_peptides))
    ab = np.ascontiguousarray(abundance, dtype=np.float64).reshape(-1)
    n = len(gid)
    assert len(plex) == n and len(n_psms) == n and len(n_peptides) == n and len(ab) == n * len(headers)
    hs = (C.c_char_p * max(len(headers), 1))(*[h.encode() for h in headers])
    ns = (C.c_char_p * max(n, 1))(*[names[int(g)].encode() for g in gid])
    L.check(L.load().sage_hip_write_tmt_rollup(path.encode(), first_header.encode(), hs, len(headers), n, ns, L.as_ptr(plex, C.c_uint32),
                                               L.as_ptr(n_psms, C.c_uint32), L.as_ptr(n_peptides, C.c_uint32), L.as_ptr(ab, C.c_double)))
    return n


PURITY_HEADERS = ["psm_id", "filename", "scannr", "charge", "ms1_scannr", "isolation_lo", "isolation_hi", "peaks_in_window",
                  "peaks_matched", "total_intensity", "precursor_intensity", "below_intensity", "purity"]


def purity_rows(psm_ids, filenames: Sequence[str], file_id, spec_ids, charge, ms1_ids, isolation_lo, isolation_hi, result) -> List[List[str]]:
    """purity.sage.tsv's rows for a PurityResult-like object: one per reported PSM in the order given.  ms1_ids: the
    id of the MS1 scan used, "" or None where there is none; isolation_lo / isolation_hi: the pair used (f32)."""
    lo, hi = np.asarray(isolation_lo, dtype=np.float32), np.asarray(isolation_hi, dtype=np.float32)
    return [[str(int(psm_ids[r])), filenames[int(file_id[r])], spec_ids[r], str(int(charge[r])), ms1_ids[r] or "", ryu_f32(lo[r]),
             ryu_f32(hi[r]), str(int(result.n_window[r])), str(int(result.n_matched[r])), ryu_f64(np.float64(result.total[r])),
             ryu_f64(np.float64(result.matched[r])), ryu_f64(np.float64(result.below[r])), ryu_f32(np.float32(result.purity[r]))]
            for r in range(len(spec_ids))]


def write_purity(path: str, rows: Sequence[List[str]]) -> None:
    with open(path, "w", newline="") as fh:
        fh.write(_record(PURITY_HEADERS) + "\n")
        for r in rows:
            fh.write(_record(r) + "\n")


def write_purity_native(path: str, psm_ids, filenames: Sequence[str], file_id, spec_ids, charge, ms1_ids, isolation_lo, isolation_hi,
                        result) -> None:
    """purity.sage.tsv through the C++ writer (sage_hip_write_purity): the bytes of purity_rows + write_purity."""
    import ctypes as C

    from . import _lib as L
    n = len(spec_ids)
    pid = np.ascontiguousarray(psm_ids, dtype=np.uint64)
    fid = np.ascontiguousarray(file_id, dtype=np.uint32)
    z = np.ascontiguousarray(charge, dtype=np.uint8)
    lo, hi = np.ascontiguousarray(isolation_lo, dtype=np.float32), np.ascontiguousarray(isolation_hi, dtype=np.float32)
    assert len(pid) == n and len(fid) == n and len(z) == n and len(lo) == n and len(hi) == n and len(ms1_ids) == n
    keep = []
    cout = result.to_c(keep)
    ids = (C.c_char_p * max(n, 1))(*[s.encode() for s in spec_ids])
    ms1 = (C.c_char_p * max(n, 1))(*[(s or "").encode() for s in ms1_ids])
    names = (C.c_char_p * max(len(filenames), 1))(*[s.encode() for s in filenames])
    L.check(L.load().sage_hip_write_purity(path.encode(), n, L.as_ptr(pid, C.c_uint64), L.as_ptr(fid, C.c_uint32), ids, L.as_ptr(z, C.c_uint8),
                                           ms1, L.as_ptr(lo, C.c_float), L.as_ptr(hi, C.c_float), C.byref(cout), names, len(filenames)))


TMT_HEADERS = ["filename", "scannr", "ion_injection_time"]


def tmt_rows(filenames: Sequence[str], file_id, spec_ids, ion_injection_time, intensity) -> List[List[str]]:
    """write_tmt (runner.rs:1140-1180): one row per quantified spectrum, in the order given; ryu f32 values."""
    inten = np.asarray(intensity, dtype=np.float32).reshape(len(spec_ids), -1) if len(spec_ids) else []
    return [[filenames[int(f)], s, ryu_f32(t)] + [ryu_f32(x) for x in row]
            for f, s, t, row in zip(file_id, spec_ids, np.asarray(ion_injection_time, dtype=np.float32), inten)]


def write_tmt(path: str, headers: Sequence[str], rows: Sequence[List[str]]) -> None:
    with open(path, "w", newline="") as fh:
        fh.write(_record(TMT_HEADERS + list(headers)) + "\n")
        for r in rows:
            fh.write(_record(r) + "\n")


def write_tmt_native(path: str, headers: Sequence[str], filenames: Sequence[str], file_id, spec_ids, ion_injection_time,
                     intensity) -> None:
    """tmt.tsv through the C++ writer (sage_hip_write_tmt): the bytes of tmt_rows + write_tmt."""
    import ctypes as C

    from . import _lib as L
    n = len(spec_ids)
    fid = np.ascontiguousarray(file_id, dtype=np.uint32)
    iit = np.ascontiguousarray(ion_injection_time, dtype=np.float32)
    inten = np.ascontiguousarray(intensity, dtype=np.float32).reshape(-1)
    assert len(fid) == n and len(iit) == n and len(inten) == n * len(headers)
    hs = (C.c_char_p * max(len(headers), 1))(*[h.encode() for h in headers])
    ids = (C.c_char_p * max(n, 1))(*[s.encode() for s in spec_ids])
    names = (C.c_char_p * max(len(filenames), 1))(*[s.encode() for s in filenames])
    L.check(L.load().sage_hip_write_tmt(path.encode(), hs, len(headers), n, L.as_ptr(fid, C.c_uint32), ids, L.as_ptr(iit, C.c_float),
                                        L.as_ptr(inten, C.c_float), names, len(filenames)))
