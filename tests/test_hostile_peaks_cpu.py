"""Hostile peak lists (tests/hostile_peaks.py) on the CPU, before tests/test_gpu_hostile_peaks.py feeds them to the device:

  * the census of the batches holds and is the one filed in profiles/hostile_peaks_census.json;
  * the host restatement of SpectrumProcessor::process (host_db.cpp, what `--host-preprocess` runs) equals the oracle on every class,
    masses and intensities as uint32 BITS (assert_array_equal calls any two NaNs equal: a -NaN for a +NaN would pass it);
  * the processed lists go through the host emulation of the device's peak readers (tests/hostemu/core_emu.cpp, core.h's own
    code): select_most_intense_peak in its three forms against an independent restatement, the peak-presence bitmap, the position
    tables' windows; the hostile precursors through scalar_query_window (tests/hostemu/prelim_window_emu.cpp).

The oracle against the second reading on the same batches: tests/test_scoring_second_reading.py."""
import ctypes as C
import json

import numpy as np
import pytest

import hostile_peaks as H
import oracle_lib
import raw_spectra as G
import second_reading as SR
import tmt_reference as T
from sage_amd.api import DatabaseParameters, RawSpectrum, ScorerParams, SpectrumBatch, SpectrumProcessor
from test_core_emulation import emu, fp  # noqa: F401  (the fixture that builds tests/hostemu)
from test_prelim_window_emulation import emu as window_emu, numpy_window  # noqa: F401

F32 = np.float32
u32p = C.POINTER(C.c_uint32)
f32p = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def fresh_census():
    c = H.census()
    H.assert_census(c)     # before any comparison
    return c


def test_census(fresh_census):
    print(json.dumps(fresh_census["preprocessing"]))
    with open(H.CENSUS_FILE) as f:
        assert json.load(f) == fresh_census, "profiles/hostile_peaks_census.json is not this census (python tests/hostile_peaks.py)"


def assert_same_bits(got, want, context):
    """(masses, intensities, tic): masses and intensities bit for bit (a NaN: NaN-ness and sign), the total ion current by bits
    when finite and by NaN-ness otherwise (it orders nothing and prints as NaN)"""
    gm, gi, gt = got
    wm, wi, wt = want
    assert len(gm) == len(wm), f"{context}: {len(gm)} peaks vs oracle {len(wm)}"
    for name, a, b in (("masses", gm, wm), ("intensities", gi, wi)):
        a, b = H.bits(a), H.bits(b)
        if not np.array_equal(a, b):
            k = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{context}: {name}[{k}] = {a[k]:#010x} vs oracle {b[k]:#010x} ({int((a != b).sum())} of {len(a)} differ)")
    gt, wt = F32(gt), F32(wt)
    assert (np.isnan(gt) and np.isnan(wt)) or H.bits(gt)[0] == H.bits(wt)[0], f"{context}: total ion current {gt!r} vs oracle {wt!r}"


# ---- a. preprocessing: host restatement == oracle ---------------------------------------------------------------------------------
CASES_PER_CELL = 215   # x 7 classes x 2 modes = 3 010 spectra


@pytest.mark.parametrize("deisotope", [True, False], ids=["deisotope", "heap"])
@pytest.mark.parametrize("cls", H.CLASSES)
def test_host_processing_matches_the_oracle_bit_for_bit(fresh_census, cls, deisotope):
    seen_nan = 0
    for k in range(CASES_PER_CELL):
        rng = np.random.default_rng([H.CLASSES.index(cls), int(deisotope), k, 77])
        n = G.peak_count(rng, huge=0.005)
        mz, it = H.hostile(rng, cls, *G.raw_peaks(rng, n))
        z = G.precursor_charge(rng)
        top_n = G.take_top_n(rng, n)
        min_mz = G.min_deisotope_mz(rng, [mz[np.isfinite(mz)]])
        ctx = f"{cls} case {k}: n={n} z={z} take_top_n={top_n} min_deisotope_mz={min_mz!r}"
        p = SpectrumProcessor(top_n, deisotope, min_mz).process(RawSpectrum(mz, it, 500.0, z or None))
        want = oracle_lib.process_ms2(top_n, deisotope, min_mz, mz, it, z)
        assert_same_bits((p.masses, p.intensities, p.total_ion_current), want, ctx)
        seen_nan += int(np.isnan(want[0]).any() or np.isnan(want[1]).any() or np.isnan(F32(want[2])))
    if cls in ("mz_special", "it_special", "both_inf", "all_nan", "everything"):
        assert seen_nan > 10, f"{cls}: {seen_nan} spectra with a NaN"


def test_a_created_nan_has_its_sign_set():
    """The contract of the envelope sum: inf + -inf is the x86-64 default NaN 0xFFC00000 in the oracle and in the host restatement,
    f32::total_cmp sorts it below -inf and the top-N cut drops it first."""
    mz = np.array([500.0, 500.0 + float(H.NEUTRON), 700.0, 800.0], F32)
    it = np.array([np.inf, -np.inf, 5.0, -np.inf], F32)
    for process in (lambda *a: oracle_lib.process_ms2(*a),
                    lambda n, d, m, x, y, z: (lambda p: (p.masses, p.intensities, p.total_ion_current))(
                        SpectrumProcessor(n, d, m).process(RawSpectrum(x, y, 500.0, z)))):
        m, i, tic = process(150, True, 0.0, mz, it, 2)
        assert H.bits(i).tolist() == [0xFFC00000, H.bits(F32(5.0))[0], H.bits(F32(-np.inf))[0]] and np.isnan(F32(tic))
        m, i, _ = process(2, True, 0.0, mz, it, 2)       # the cut keeps 5.0 and -inf: the created NaN goes first
        assert H.bits(i).tolist() == [H.bits(F32(5.0))[0], H.bits(F32(-np.inf))[0]]


# ---- b. the device's peak readers, through their host emulation ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scored(fresh_census):
    """the scored batches' processed spectra, the peptides and the oracle's PSMs (the ions the rescoring kernels look up)"""
    dbp = DatabaseParameters(**H.TRYPTIC)
    db = dbp.build(H.fasta_text())
    orc = oracle_lib.OracleDb.from_product(db)
    peps = SR.Peptides(orc.arrays())
    out = []
    for deisotope in (True, False):
        raws, names = H.peak_spectra(db)
        spectra = H.oracle_processed(raws, 150, deisotope)
        feats, counts, _, _ = orc.score(ScorerParams(report_psms=2, min_matched_peaks=2), SpectrumBatch.from_spectra(spectra))
        out.append((spectra, names, feats, counts))
    return db, peps, out


TOLS = [("ppm", -10.0, 10.0), ("da", -0.02, 0.01), ("ppm", -50.0, 20.0), ("pct", -0.001, 0.001)]
KINDS = {"ppm": 0, "pct": 1, "da": 2}
# (no centre of -0.0: the reference adds `offset.unwrap_or_default()`, +0.0, to both bounds (spectrum.rs:143-146), which turns a
# bound of -0.0 into +0.0; core.h, the oracle and the second reading state the search "with offset == None" without that addition.
# A bound is -0.0 only for a centre of -0.0, and a fragment m/z — a sum of residue masses over a charge — is never that.)
SPECIAL_CENTRES = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -300.0, 3e38, -3e38, 1e-30]


def _centres(peps, feats, count, masses, rng):
    c = list(SPECIAL_CENTRES) + list(rng.uniform(-50.0, 3000.0, 10))
    finite = masses[np.isfinite(masses)]
    c += list(finite[:: max(1, len(finite) // 25)])                                    # on a peak: matches
    for r in range(int(count)):                                                         # the PSMs' own ion ladders, charges 1-3
        for kind in (SR.B, SR.Y):
            s = peps.ion_series(int(feats[r]["peptide_idx"]), kind)
            c += [x / F32(z) for x in s for z in (1, 2, 3)]
    return np.asarray(c, F32)


def test_select_most_intense_peak_readers_on_hostile_lists(emu, scored):  # noqa: F811
    _, peps, batches = scored
    rng = np.random.default_rng(5)
    checked = matched = nan_first = nan_last = 0
    for spectra, names, feats, counts in batches:
        for i, s in enumerate(spectra):
            m, it = np.ascontiguousarray(s.masses, F32), np.ascontiguousarray(s.intensities, F32)
            P = len(m)
            keys = H.total_key(m)
            assert np.all(keys[1:] >= keys[:-1]), f"{s.id}: processed masses are not ascending in the total order"
            nan_first += int(P > 0 and H.bits(m[:1])[0] == 0xFFC00000)
            nan_last += int(P > 0 and H.bits(m[-1:])[0] == 0x7FC00000)
            mb, ib = (m, it) if P else (np.zeros(1, F32), np.zeros(1, F32))
            tol = TOLS[i % len(TOLS)]
            for c in _centres(peps, feats[i], counts[i], m, rng):
                want = T.select_most_intense_peak(m, it, c, tol)
                want = -1 if want is None else int(want)
                assert SR.select_most_intense_peak(m, it, c, tol) == (None if want < 0 else want)
                got = [emu.emu_select_peak(fp(mb), fp(ib), P, float(c), KINDS[tol[0]], tol[1], tol[2], 0),
                       emu.emu_select_peak(fp(mb), fp(ib), P, float(c), KINDS[tol[0]], tol[1], tol[2], 1),
                       emu.emu_select_peak_lut(fp(mb), fp(ib), P, float(c), KINDS[tol[0]], tol[1], tol[2])]
                assert all(-1 <= g < max(P, 0) or g == -1 for g in got), (s.id, float(c), got, P)
                assert got == [want] * 3, f"{s.id} ({names[i]}), centre {float(c)!r}, {tol}: scan / lockstep / table {got}, restatement {want}"
                checked += 1
                matched += want >= 0
    assert checked > 10000 and matched > 2000 and nan_first > 5 and nan_last > 5, (checked, matched, nan_first, nan_last)


def test_peak_bitmap_never_drops_a_match_on_hostile_lists(emu, scored):  # noqa: F811
    _, peps, batches = scored
    rng = np.random.default_rng(6)
    total_match = active = inactive = 0
    for spectra, names, feats, counts in batches:
        for i, s in enumerate(spectra):
            m = np.ascontiguousarray(s.masses, F32)
            if not len(m):
                continue
            ions = _centres(peps, feats[i], counts[i], m, rng)
            # (the hostile values here are the PEAKS'.  An ion of 2^28 Da and more saturates pbm_index, and from 3.4e37 on its ppm
            # window overflows to [-inf, +inf] and "matches" every peak: a matter of hostile databases, not of this module)
            ions = ions[~(np.abs(ions) >= 2.0 ** 28)]
            with np.errstate(all="ignore"):
                ions = np.concatenate([ions, ions * F32(2.0), ions * F32(3.0)]).astype(F32)   # (ion / charge lands on the peaks)
            for kind, lo, hi in TOLS:
                n_match, n_set, act = C.c_uint32(), C.c_uint32(), C.c_int()
                bad = emu.emu_peak_bitmap_violations(fp(m), len(m), KINDS[kind], lo, hi, fp(ions), len(ions), C.byref(n_match),
                                                     C.byref(n_set), C.byref(act))
                if bad:  # name the ions
                    one = [float(x) for x in ions if emu.emu_peak_bitmap_violations(
                        fp(m), len(m), KINDS[kind], lo, hi, fp(np.array([x], F32)), 1, C.byref(n_match), C.byref(n_set), C.byref(act))]
                    raise AssertionError(f"{s.id} ({names[i]}), {kind} {lo} {hi}: the bitmap says 'no match' for matches of ions {one}")
                hostile_mass = bool((~np.isfinite(m)).any() or (m < 0).any() or (m >= 8388608.0).any())
                assert act.value == (0 if hostile_mass else 1) or kind != "ppm", (s.id, act.value)
                total_match += n_match.value
                active += act.value
                inactive += 1 - act.value
    assert total_match > 5000 and active > 50 and inactive > 50, (total_match, active, inactive)


def test_position_table_windows_of_hostile_peaks(emu, scored):  # noqa: F811
    """the windows prelim_kernel asks the tiles' position tables for: Tolerance::bounds(mass x charge) of every processed peak —
    NaN, infinite (3e38 x 2), negative and zero bounds among them; no entry inside a window may lie outside its run"""
    db, _, batches = scored
    frag = np.sort(np.ascontiguousarray(db.fragments["fragment_mz"][:: max(1, len(db.fragments) // 4000)], F32))
    top = float(frag[-1])
    n_windows = degenerate = 0
    for scale in (32.0, 256.0):
        stride = int(np.ceil(top * scale)) + 3
        for spectra, _, _, _ in batches:
            masses = np.concatenate([s.masses for s in spectra]).astype(F32)
            for kind, tlo, thi in TOLS[:2]:
                los, his = [], []
                with np.errstate(all="ignore"):
                    for z in (1, 2, 3):
                        for mass in masses:
                            lo, hi = T.bounds(F32(mass) * F32(z), (kind, tlo, thi))
                            los.append(lo), his.append(hi)
                los, his = np.asarray(los, F32), np.asarray(his, F32)
                run = C.c_uint64()
                assert emu.emu_lut_windows(fp(frag), len(frag), scale, stride, fp(los), fp(his), len(los), C.byref(run)) == 0
                n_windows += len(los)
                degenerate += int((~np.isfinite(los) | ~np.isfinite(his) | (his < 0)).sum())
    assert n_windows > 50000 and degenerate > 1000, (n_windows, degenerate)


def test_precursor_windows_of_hostile_precursors(window_emu, scored):  # noqa: F811
    """scalar_query_window (what a resident batch's upload leaves in the schedule records) on the hostile precursors: m/z NaN,
    +-inf, 0, -500, 3e38 and PROTON at charges 1-4, isotope errors -1..3, ppm / Da / wide-window tolerances"""
    db, _, _ = scored
    mono = np.ascontiguousarray(db.pep_mono, F32)
    raws, touched = H.precursor_spectra(db)
    out = np.zeros(4, np.uint32)
    checked = hostile = nonempty = 0
    with np.errstate(all="ignore"):
        for r, t in zip(raws, touched):
            for z in (1, 2, 3, 4):
                for iso in (-1, 0, 1, 3):
                    mass = (F32(r.precursor_mz) - H.PROTON) * F32(z) - F32(iso) * H.NEUTRON
                    for tol in (("ppm", -10.0, 10.0), ("da", -3.0, 3.0), ("ppm", -50.0, 50.0), ("da", -6.0 * z, 6.0 * z)):
                        plo, phi = T.bounds(mass, tol)
                        window_emu.emu_scalar_query_window(mono.ctypes.data_as(f32p), len(mono), float(plo), float(phi), out.ctypes.data_as(u32p))
                        want = numpy_window(mono, plo, phi)
                        assert out.tolist() == want, (r.id, float(r.precursor_mz), z, iso, tol, out.tolist(), want)
                        assert out[0] <= len(mono) and out[1] <= len(mono) and out[3] <= len(mono)
                        a, b = SR.binary_search_slice(mono, plo, phi)
                        assert (a, b) == (want[0], want[1])
                        checked += 1
                        hostile += bool(t)
                        nonempty += want[3] > want[2]
    assert checked > 2000 and hostile > 1000 and nonempty > 300, (checked, hostile, nonempty)
