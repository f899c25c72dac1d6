"""Sequential restatement of sage-core's label-free quantification for ion-mobility MS1 spectra: what v0.15 adds to lfq.rs
(build_feature_map's mobility window, lfq.rs:111-127; the per-spectrum choice of lookup, :267-286; mass_mobility_lookup,
:677-686), spectrum.rs:344-378 (the MS1 sort that carries the mobility column) and mass.rs:28-32 (Tolerance::Pct).  The checker
of sage_hip_lfq_im.  Everything else — the sort keys, mass_lookup, Grid::add_entry, integration, picked_precursor — is
tests/lfq_reference.py, imported unchanged; the orders that file fixes hold here too: a mobility filter only removes matches.
f32 arithmetic on np.float32 scalars (IEEE single, no contraction)."""
import numpy as np

import lfq_reference as R
from lfq_reference import F32, GRID_SIZE, N_ISOTOPES, PROTON, RT_TOL, total_key


def tol_bounds_pct(center, pct):
    """Tolerance::Pct(-pct, pct).bounds(center) (mass.rs:28-32): center * lo / 100.0, then center + delta, f32."""
    c, lo, hi = F32(center), -F32(pct), F32(pct)
    with np.errstate(all="ignore"):
        return c + c * lo / F32(100.0), c + c * hi / F32(100.0)


def select_mobility(feats: dict, settings: dict) -> dict:
    """The `ims` of the feature build_feature_map keeps per peptide (lfq.rs:100-105: the first one in confidence order with
    peptide_q <= peptide_q_value and label == 1 — the rule of lfq_reference.select_features)."""
    thr = F32(settings["peptide_q_value"])
    ims = {}
    for j in range(len(feats["peptide_idx"])):
        if F32(feats["peptide_q"][j]) <= thr and int(feats["label"][j]) == 1:
            ims.setdefault(int(feats["peptide_idx"][j]), F32(feats["ims"][j]))
    return ims


def build_feature_map(settings: dict, precursor_charge, feats: dict):
    """lfq.rs:94-193: lfq_reference.build_feature_map, every window with the (mobility_lo, mobility_hi) of its peptide's
    feature — the charge x isotope x forward / decoy windows inherit them unchanged (`..range`, `..fwd`)."""
    fmap = R.build_feature_map(settings, precursor_charge, feats)
    ims = select_mobility(feats, settings)
    bounds = {p: tol_bounds_pct(v, settings["mobility_pct_tolerance"]) for p, v in ims.items()}
    for e in fmap["ranges"]:
        e["mobility_lo"], e["mobility_hi"] = bounds[e["peptide"]]
    return fmap


def process_ms1(mz, intensity, mobility):
    """SpectrumProcessor::process for an MS1 spectrum with mobility (spectrum.rs:344-378): (mz - PROTON, intensity, mobility)
    sorted stably by mass (total_cmp), all three columns."""
    m = np.asarray(mz, dtype=np.float32) - PROTON
    order = sorted(range(len(m)), key=lambda i: total_key(m[i]))
    return m[order], np.asarray(intensity, dtype=np.float32)[order], np.asarray(mobility, dtype=np.float32)[order]


def mass_mobility_lookup(fmap, rt, mass, mobility):
    """Query::mass_mobility_lookup (lfq.rs:677-686)."""
    for e in R.mass_lookup(fmap, rt, mass):
        if e["mobility_hi"] >= mobility and e["mobility_lo"] <= mobility:
            yield e


def trace(fmap, spectra, alignments, n_files: int, combine: bool, isotopes_of):
    """FeatureMap::quantify's tracing pass (lfq.rs:239-287).  spectra: (file_id, scan_start_time, masses, intensities,
    mobilities or None) of processed MS1 spectra in order; a spectrum without mobilities (`mobilities.is_empty()`) goes through
    mass_lookup.  Returns {key: grid}."""
    grids = {}
    step = (RT_TOL * F32(2.0)) / F32(GRID_SIZE)
    for file_id, sst, masses, ints, mobs in spectra:
        rt = R.spectrum_rt(sst, alignments[file_id])
        for i, (mass, inten) in enumerate(zip(masses, ints)):
            if mobs is None or len(mobs) == 0:
                matches = R.mass_lookup(fmap, rt, F32(mass))
            else:
                matches = mass_mobility_lookup(fmap, rt, F32(mass), F32(mobs[i]))
            for e in matches:
                k = R.grid_key(e, combine)
                g = grids.get(k)
                if g is None:
                    g = grids[k] = dict(rt_min=e["rt"] - RT_TOL, rt_step=step, ref=e["file_id"], dist=isotopes_of(e["peptide"]),
                                        matrix=np.zeros((n_files * N_ISOTOPES, GRID_SIZE), dtype=np.float64))
                R.add_entry(g, rt, e["isotope"], file_id, F32(inten))
    return grids


def quantify(settings, precursor_charge, feats, spectra, alignments, n_files, isotopes_of, grids=None):
    """The LFQ block of runner.rs:562-575 for spectra with mobility.  Returns (results {key: dict}, passing, grids)."""
    if grids is None:
        fmap = build_feature_map(settings, precursor_charge, feats)
        grids = trace(fmap, spectra, alignments, n_files, settings["combine_charge_states"], isotopes_of)
    return R.quantify(settings, precursor_charge, None, None, None, n_files, None, grids=grids)
