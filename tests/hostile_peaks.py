"""Seeded HOSTILE peak lists, and a census of what they make the preprocessing and the scoring meet — TEST INFRASTRUCTURE.

The MGF reader takes `inf`, `-Infinity` and `nan` and keeps peaks in file order, and nothing between the reader and the kernels
looks at a value: process_kernel (process.hip) replays deisotope and the heap on whatever it is given, and the scoring kernels
read the masses it leaves.  This module draws such input — classes applied to a tests/raw_spectra.py spectrum (preprocessing) or
to a sage_amd.synthetic.synthetic_spectra one (scoring; the hostile values land on ladder peaks as well as on noise):

  unsorted     a random permutation of the peaks
  descending   m/z in descending order
  mz_special   m/z from +-NaN, +-inf, +-0.0, -300, PROTON exactly (mass 0), 3e38
  it_special   intensities from +-NaN, +inf, -0.0, 0.0, -50
  both_inf     +inf and -inf intensities in one spectrum, an envelope pair (+inf parent, -inf satellite) among them: the only
               class in which ARITHMETIC creates NaNs (inf + -inf in deisotope's `+=` and in the total ion current)
  all_nan      every m/z a NaN
  everything   the union of the above without both_inf

and hostile precursors (m/z NaN, +-inf, 0, -500, 3e38, PROTON) on every second spectrum of a scoring batch.

Only the two default quiet NaNs are fed: 0x7FC00000 and 0xFFC00000.  Other payloads and signalling NaNs are out of scope: what
an addition makes of them differs between x86-64 and gfx950 by more than a sign and no reader of this project produces them.

NaN rule the tests hold the device to: a NaN that is COPIED keeps its bits; a NaN that an addition CREATES from two non-NaN
operands in deisotope's envelope sum is the x86-64 default NaN 0xFFC00000 (sign set) — the oracle's value on the reference's
platform, which f32::total_cmp sorts below -inf, so the top-N cut drops it; the total ion current orders nothing and is compared by
NaN-ness.

Nothing here is shared with the product code: the expected values come from the oracle (oracle_lib.process_ms2, OracleDb.score).
`python tests/hostile_peaks.py` writes the census to profiles/hostile_peaks_census.json; tests/test_hostile_peaks_cpu.py holds
the file to a fresh census."""
import json
import os

import numpy as np

import raw_spectra as G

F32 = np.float32
PROTON = F32(1.0072764)
NEUTRON = F32(1.00335)
CLASSES = ("unsorted", "descending", "mz_special", "it_special", "both_inf", "all_nan", "everything")
CENSUS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hostile_peaks_census.json")


def _bits(u):
    return np.array([u], np.uint32).view(F32)[0]


PNAN, NNAN = _bits(0x7FC00000), _bits(0xFFC00000)
MZ_SPECIALS = np.array([PNAN, NNAN, np.inf, -np.inf, 0.0, -0.0, -300.0, PROTON, 3e38], F32)
IT_SPECIALS = np.array([PNAN, NNAN, np.inf, -0.0, 0.0, -50.0], F32)
PRECURSOR_SPECIALS = np.array([PNAN, NNAN, np.inf, -np.inf, 0.0, -500.0, 3e38, PROTON], F32)


def total_key(x):
    """f32::total_cmp as int64 keys (stated on the bit patterns)"""
    b = np.asarray(x, F32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _some(rng, n, frac):
    """indices of about frac * n peaks, at least one (none of an empty spectrum)"""
    k = np.flatnonzero(rng.random(n) < frac)
    return k if len(k) or n == 0 else rng.integers(0, n, 1)


def hostile(rng, cls, mz, it, frac=0.08):
    """(mz, intensity) of class `cls` from an ordinary spectrum (copies; f32)"""
    mz, it = np.array(mz, F32), np.array(it, F32)
    n = len(mz)
    if cls in ("mz_special", "everything"):
        k = _some(rng, n, frac)
        mz[k] = rng.choice(MZ_SPECIALS, len(k))
    if cls in ("it_special", "everything"):
        k = _some(rng, n, frac)
        it[k] = rng.choice(IT_SPECIALS, len(k))
    if cls == "all_nan":
        mz[:] = np.where(rng.random(n) < 0.5, PNAN, NNAN)
    if cls == "both_inf" and n:
        # an envelope pair: a +inf parent and a -inf satellite one neutron above it (charge 1: every precursor charge admits it);
        # deisotope adds the satellite to the parent (-inf < +inf), inf + -inf
        pairs = max(1, n // 200)
        parents = rng.integers(0, n, pairs)
        it[parents] = np.inf
        mz = np.concatenate([mz, (mz[parents] + NEUTRON).astype(F32)])
        it = np.concatenate([it, np.full(pairs, -np.inf, F32)])
        if len(mz) > n and n > 1:   # the peak count stays what was asked for: drop peaks that are no part of a pair
            free = np.setdiff1d(np.arange(n), parents)
            drop = rng.choice(free, min(pairs, len(free)), replace=False)
            keep = np.setdiff1d(np.arange(len(mz)), drop)
            mz, it = mz[keep], it[keep]
        others = _some(rng, len(mz), frac / 2)
        others = others[np.isfinite(it[others])]
        it[others] = np.where(rng.random(len(others)) < 0.5, np.inf, -np.inf).astype(F32)
        o = np.argsort(mz, kind="stable")
        mz, it = mz[o], it[o]
    if cls == "descending" or (cls == "everything" and rng.random() < 0.3):
        o = np.argsort(total_key(mz), kind="stable")[::-1]
        mz, it = mz[o], it[o]
    elif cls in ("unsorted", "everything"):
        o = rng.permutation(len(mz))
        mz, it = mz[o], it[o]
    return np.ascontiguousarray(mz, F32), np.ascontiguousarray(it, F32)


# ---- preprocessing batches: one per class and mode -----------------------------------------------------------------------------
N_RANDOM = 16   # spectra beside the edge counts


def preprocessing_batch(cls, deisotope):
    """About 30 raw spectra of class `cls`: every G.EDGE_COUNTS count (0 … 4 097, both sides of PROCESS_LDS_PEAKS) and N_RANDOM
    smaller ones, sizes shuffled.  Returns (spectra [(mz, intensity, precursor charge or 0)], take_top_n, min_deisotope_mz,
    min_peaks)."""
    rng = np.random.default_rng([CLASSES.index(cls), int(deisotope), 20261])
    counts = list(G.EDGE_COUNTS) + [int(c) for c in rng.integers(3, 700, N_RANDOM)]
    spectra = []
    for n in counts:
        mz, it = G.raw_peaks(rng, n)
        mz, it = hostile(rng, cls, mz, it)
        assert len(mz) == n or (cls == "both_inf" and n == 1)
        spectra.append((mz, it, G.precursor_charge(rng)))
    order = rng.permutation(len(spectra))
    if np.all(np.diff([len(spectra[i][0]) for i in order]) >= 0):
        order = order[::-1]
    spectra = [spectra[i] for i in order]
    # the cut binds for some spectra and not for others; both_inf keeps a setting under which +inf and -inf survive together
    top_n = int(rng.choice([64, 150, 150, 65535])) if cls != "both_inf" else int(rng.choice([150, 65535]))
    min_mz = G.min_deisotope_mz(rng, [s[0][np.isfinite(s[0])] for s in spectra]) if cls != "both_inf" else 0.0
    min_peaks = int(rng.choice([0, 15]))
    return spectra, top_n, min_mz, min_peaks


# ---- scoring batches -------------------------------------------------------------------------------------------------------------
TRYPTIC = dict(bucket_size=1024, enzyme=dict(missed_cleavages=1, min_len=5, max_len=50, cleave_at="KR", restrict="P"),
               static_mods={"C": 57.0215}, variable_mods={"M": [15.9949], "[": [42.010565]}, max_variable_mods=2)
FASTA = dict(n_proteins=300, seed=14)
N_PEAK_SPECTRA, PEAK_SEED = 60, 141
N_PRECURSOR_SPECTRA, PRECURSOR_SEED = 40, 142
# a scored batch mixes the classes spectrum by spectrum; all_nan (which can have no PSM) twice in 60
NAN_RUN = 40   # -NaN m/z added to every twelfth spectrum (an mz_special one)
SCORED_CLASSES = ("unsorted", "descending", "mz_special", "it_special", "both_inf", "everything")


def fasta_text():
    from sage_amd.synthetic import synthetic_fasta
    return synthetic_fasta(**FASTA)


def peak_spectra(db, chimeric=1):
    """N_PEAK_SPECTRA synthetic spectra over `db` (ladder intensities raised, as tests/test_process_fuzz.py does, so that the ladder
    survives the top-N cut), each of one hostile class.  Returns ([RawSpectrum], [class name])."""
    from sage_amd.api import RawSpectrum
    from sage_amd.synthetic import synthetic_spectra
    rng = np.random.default_rng([PEAK_SEED, chimeric])
    kw = dict(chimeric=chimeric, isolation_half_width=6.0) if chimeric > 1 else {}
    out, names = [], []
    for k, r in enumerate(synthetic_spectra(db, N_PEAK_SPECTRA, PEAK_SEED, **kw)):
        cls = "all_nan" if k % 30 == 29 else SCORED_CLASSES[k % len(SCORED_CLASSES)]
        mz, it = hostile(rng, cls, r.mz, r.intensity * F32(50.0))
        if k % 12 == 2:
            # a long run of -NaN masses in FRONT of the processed list (they survive the cut): a partition point taken in float
            # order instead of f32::total_cmp goes wrong as soon as a probe lands in the run
            at = rng.integers(0, len(mz) + 1, NAN_RUN)
            mz = np.insert(mz, at, NNAN)
            it = np.insert(it, at, F32(np.max(it[np.isfinite(it)])))
        out.append(RawSpectrum(mz, it, r.precursor_mz, r.precursor_charge, r.isolation_window, r.scan_start_time, None, 0, f"{cls}{k}"))
        names.append(cls)
    return out, names


def precursor_spectra(db, annotate_charge=True):
    """N_PRECURSOR_SPECTRA ordinary synthetic spectra; every second one has a hostile precursor m/z.  Returns ([RawSpectrum],
    touched[bool])."""
    from sage_amd.api import RawSpectrum
    from sage_amd.synthetic import synthetic_spectra
    out = []
    touched = np.arange(N_PRECURSOR_SPECTRA) % 2 == 1
    for k, r in enumerate(synthetic_spectra(db, N_PRECURSOR_SPECTRA, PRECURSOR_SEED, annotate_charge=annotate_charge,
                                            isolation_half_width=3.0)):
        pmz = float(PRECURSOR_SPECIALS[(k // 2) % len(PRECURSOR_SPECIALS)]) if touched[k] else r.precursor_mz
        z = r.precursor_charge if k % 4 < 2 else None   # known and unknown, among the touched and among the others
        out.append(RawSpectrum(r.mz, r.intensity, pmz, z, r.isolation_window, r.scan_start_time, None, 0, f"p{k}"))
    return out, touched


def oracle_processed(raws, top_n=150, deisotope=True, min_mz=0.0):
    """[ProcessedSpectrum] by the oracle's SpectrumProcessor::process"""
    import oracle_lib
    from sage_amd.api import ProcessedSpectrum
    out = []
    for r in raws:
        m, i, tic = oracle_lib.process_ms2(top_n, deisotope, min_mz, r.mz, r.intensity, r.precursor_charge)
        out.append(ProcessedSpectrum(m, i, tic, r.precursor_mz, r.precursor_charge, r.isolation_window, r.scan_start_time,
                                     r.inverse_ion_mobility, r.file_id, r.id))
    return out


def scorer_settings():
    """name -> (ScorerParams keywords, chimeric sources of the batch, precursor charge annotated): the searches the hostile
    batches go through, on the CPU against the second reading and on the device against the oracle"""
    from sage_amd.api import Tolerance
    return {
        "narrow": (dict(), 1, True),
        "chimera": (dict(chimera=True, report_psms=3, min_matched_peaks=2), 1, True),
        "da3_report5": (dict(precursor_tol=Tolerance("da", -3.0, 3.0), report_psms=5), 1, True),
        "isotope_errors": (dict(min_isotope_err=-1, max_isotope_err=3, precursor_tol=Tolerance("ppm", -50.0, 50.0), report_psms=2,
                                min_matched_peaks=2), 1, True),
        "wide_window_chimera": (dict(wide_window=True, chimera=True, report_psms=3), 2, False),
        "da_fragments": (dict(fragment_tol=Tolerance("da", -0.02, 0.01), report_psms=2), 1, True),
    }


MIN_PEAK_FRACTION = 2.0 / 3.0       # of a peak-class batch's spectra have a PSM in the oracle
MIN_PRECURSOR_FRACTION = 0.5        # of the spectra whose precursor was left alone


# ---- the census --------------------------------------------------------------------------------------------------------------------
def census_of_processed(raw_it, pm, pi, tic, created_possible):
    """what one processed spectrum adds to the census (a dict of 0 / 1 flags and counts)"""
    nan_m = np.isnan(pm)
    raw_nan, kept_nan = int(np.isnan(raw_it).sum()), int(np.isnan(pi).sum())
    return dict(
        starts_with_negative_nan_mass=int(len(pm) > 0 and bits(pm[:1])[0] == 0xFFC00000),
        ends_with_positive_nan_mass=int(len(pm) > 0 and bits(pm[-1:])[0] == 0x7FC00000),
        holds_infinite_masses=int(np.isinf(pm).any()),
        holds_negative_masses=int((pm[~nan_m] < 0).any()),
        nan_intensity_peaks_kept=0 if created_possible else kept_nan,
        nan_intensity_peaks_dropped=0 if created_possible else raw_nan - kept_nan,
        envelope_sums_that_became_nan=kept_nan if created_possible and raw_nan == 0 else 0,
        nan_tic=int(np.isnan(F32(tic))))


def preprocessing_census():
    import oracle_lib
    total, big = {}, {}
    for cls in CLASSES:
        big[cls] = 0
        for deisotope in (True, False):
            spectra, top_n, min_mz, _ = preprocessing_batch(cls, deisotope)
            big[cls] += sum(len(s[0]) > G.LDS_PEAKS for s in spectra)
            for mz, it, z in spectra:
                pm, pi, tic = oracle_lib.process_ms2(top_n, deisotope, min_mz, mz, it, z)
                c = census_of_processed(it, pm, pi, tic, cls == "both_inf" and deisotope)
                for k, v in c.items():
                    total[k] = total.get(k, 0) + v
    total["spectra_over_2048_raw_peaks_by_class"] = big
    return total


def scoring_census():
    """over the scored batches: PSM counts per setting and the non-finite Feature fields"""
    import oracle_lib
    from sage_amd.api import DatabaseParameters, ScorerParams, SpectrumBatch
    dbp = DatabaseParameters(**TRYPTIC)
    fasta = fasta_text()
    db = dbp.build(fasta)
    orc = oracle_lib.OracleDb.from_product(db)
    out = {}
    for name, (kw, chimeric, annotated) in scorer_settings().items():
        for deisotope in (True, False):
            raws, _ = peak_spectra(db, chimeric)
            if not annotated:
                for r in raws:
                    r.precursor_charge = None
            batch = SpectrumBatch.from_spectra(oracle_processed(raws, 150, deisotope))
            p = ScorerParams(**kw)
            of, oc, _, _ = orc.score(p, batch)
            f = of[np.arange(of.shape[1])[None, :] < oc[:, None]]
            out[f"{name}/{'deisotope' if deisotope else 'heap'}"] = dict(
                spectra=batch.n, spectra_with_psm=int((oc > 0).sum()), psms=int(oc.sum()),
                psms_with_non_finite_ms2_intensity=int((~np.isfinite(f["ms2_intensity"])).sum()),
                psms_with_non_finite_matched_intensity_pct=int((~np.isfinite(f["matched_intensity_pct"])).sum()))
        raws, touched = precursor_spectra(db, annotated)
        batch = SpectrumBatch.from_spectra(oracle_processed(raws))
        of, oc, _, _ = orc.score(ScorerParams(**kw), batch)
        out[f"{name}/precursors"] = dict(spectra=batch.n, untouched=int((~touched).sum()),
                                         untouched_with_psm=int((oc[~touched] > 0).sum()), psms=int(oc.sum()),
                                         psms_of_touched=int(oc[touched].sum()))
    return out


def census():
    return json.loads(json.dumps(dict(preprocessing=preprocessing_census(), scoring=scoring_census())))


def assert_census(c):
    """every condition the hostile tests rest on — asserted before any comparison"""
    p = c["preprocessing"]
    for k in ("starts_with_negative_nan_mass", "ends_with_positive_nan_mass", "holds_infinite_masses", "holds_negative_masses",
              "nan_intensity_peaks_kept", "nan_intensity_peaks_dropped", "envelope_sums_that_became_nan", "nan_tic"):
        assert p[k] > 0, f"census: {k} == 0"
    for cls in CLASSES:
        assert p["spectra_over_2048_raw_peaks_by_class"][cls] > 0, f"census: no spectrum of more than 2 048 raw peaks in {cls}"
    s = c["scoring"]
    assert sum(v.get("psms_with_non_finite_ms2_intensity", 0) for v in s.values()) > 0
    assert sum(v.get("psms_with_non_finite_matched_intensity_pct", 0) for v in s.values()) > 0
    for name, v in s.items():
        if name.endswith("/precursors"):
            assert v["untouched_with_psm"] >= MIN_PRECURSOR_FRACTION * v["untouched"], f"census: {name}: {v}"
        else:
            assert v["spectra_with_psm"] >= MIN_PEAK_FRACTION * v["spectra"], f"census: {name}: {v}"


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    figures = census()
    assert_census(figures)
    with open(CENSUS_FILE, "w") as f:
        json.dump(figures, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(figures, indent=1, sort_keys=True))
