"""Ion-mobility LFQ, the host side (CPU only): the restatement tests/lfq_im_reference.py against the reference's own known
answer; core.h's Tolerance::Pct branch against the restatement; the per-peak mobility array of MS1 spectra through both mzML
readers (csrc/mzml_reader.cpp and sage_amd/mzml.py), bit for bit; the batch plumbing that carries the column to the call."""
import ctypes as C
import re

import numpy as np
import pytest

import lfq_im_reference as RI
import lfq_reference as R
from sage_amd import _lib as L
from sage_amd.api import RawBatch, RawSpectrum
from sage_amd.mzml import MOBILITY_ARRAYS, read_mzml, read_mzml_native, write_mzml
from test_core_emulation import emu  # noqa: F401  (core.h compiled for the host)

F32 = np.float32


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_known_answer():
    """spectrum.rs:630-649 process_ms1_with_mobility_sorts_all_columns_by_mass"""
    m, it, mob = RI.process_ms1([102.0, 100.0, 101.0], [30.0, 10.0, 20.0], [3.0, 1.0, 2.0])
    assert m.tolist() == [F32(100.0) - R.PROTON, F32(101.0) - R.PROTON, F32(102.0) - R.PROTON]
    assert it.tolist() == [10.0, 20.0, 30.0] and mob.tolist() == [1.0, 2.0, 3.0]
    assert len(m) == len(it) == len(mob)
    # without the column: the unchanged path of lfq_reference gives the same masses and intensities
    m0, it0 = R.process_ms1([102.0, 100.0, 101.0], [30.0, 10.0, 20.0])
    assert np.array_equal(bits(m0), bits(m)) and np.array_equal(bits(it0), bits(it))


def test_restatement_sort_is_stable_and_total():
    """equal masses keep their order (with their mobilities); -0.0 < +0.0 < NaN in total_cmp"""
    mz = F32(500.0) + R.PROTON
    m, it, mob = RI.process_ms1([mz, F32(400.0), mz, mz], [1.0, 2.0, 3.0, 4.0], [0.9, 0.5, 0.7, 0.8])
    assert it.tolist() == [2.0, 1.0, 3.0, 4.0] and mob.tolist() == [F32(0.5), F32(0.9), F32(0.7), F32(0.8)]
    m, it, mob = RI.process_ms1([np.nan, R.PROTON, 1.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0])
    assert mob.tolist() == [3.0, 2.0, 1.0]


def test_pct_bounds_restatement_and_core_h(emu):  # noqa: F811
    """Tolerance::Pct(-t, t).bounds(ims) (mass.rs:28-32).  core.h's tol_bounds has had that branch without a caller: held to
    the restatement here, over the mobility range, the specials (0, negative, inf, NaN) and tolerance 0, before
    mobility_bounds_kernel relies on it."""
    assert RI.tol_bounds_pct(1.0, 1.0) == (F32(1.0) + F32(1.0) * F32(-1.0) / F32(100.0), F32(1.0) + F32(1.0) * F32(1.0) / F32(100.0))
    assert RI.tol_bounds_pct(0.0, 1.0) == (0.0, 0.0)
    lo, hi = RI.tol_bounds_pct(-1.0, 1.0)
    assert lo > hi  # a negative ims gives an empty window
    assert all(np.isnan(v) for v in RI.tol_bounds_pct(np.nan, 1.0))
    v = F32(0.8731)
    assert RI.tol_bounds_pct(v, 0.0) == (v, v)
    rng = np.random.default_rng(5)
    centers = np.concatenate([rng.uniform(0.3, 2.0, 3000), rng.uniform(-2.0, 2000.0, 500),
                              [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, 3e38]]).astype(np.float32)
    pcts = np.concatenate([rng.uniform(0.0, 5.0, len(centers) - 4), [0.0, 1.0, 3.0, 100.0]]).astype(np.float32)
    for c, t in zip(centers, pcts):
        a, b = C.c_float(), C.c_float()
        emu.emu_tol_bounds(1, float(-t), float(t), float(c), C.byref(a), C.byref(b))
        lo, hi = RI.tol_bounds_pct(c, t)
        assert bits(a.value) == bits(lo) and bits(b.value) == bits(hi), (c, t)


def test_restatement_lookup_filters_and_chooses_per_spectrum():
    """mass_mobility_lookup = mass_lookup filtered by hi >= m && lo <= m; a spectrum without mobilities uses mass_lookup;
    ims == 0 gives the window [0, 0]; NaN matches nothing."""
    feats = dict(peptide_idx=np.array([0, 1, 1]), label=np.array([1, 1, 1]), calcmass=np.array([1000.0, 1000.0, 1000.0], np.float32),
                 file_id=np.array([0, 0, 0]), aligned_rt=np.array([0.5, 0.5, 0.5], np.float32), peptide_q=np.zeros(3, np.float32),
                 ims=np.array([1.0, 0.0, 1.2], np.float32))  # the second feature of peptide 1 is ignored
    st = R.default_settings()
    fmap = RI.build_feature_map(st, (2, 2), feats)
    assert len(fmap["ranges"]) == 2 * 3 * 2
    for e in fmap["ranges"]:
        assert (e["mobility_lo"], e["mobility_hi"]) == (RI.tol_bounds_pct(1.0, 1.0) if e["peptide"] == 0 else (0.0, 0.0))
    mass = F32(500.0)
    hits = lambda m: sorted(e["peptide"] for e in RI.mass_mobility_lookup(fmap, F32(0.5), mass, F32(m)))
    assert sorted(e["peptide"] for e in R.mass_lookup(fmap, F32(0.5), mass)) == [0, 1]
    assert hits(1.0) == [0] and hits(0.0) == [1] and hits(-0.0) == [1] and hits(np.nan) == [] and hits(1.02) == []
    lo, hi = RI.tol_bounds_pct(1.0, 1.0)
    assert hits(lo) == [0] and hits(hi) == [0] and hits(np.nextafter(lo, F32(-9))) == [] and hits(np.nextafter(hi, F32(9))) == []
    al = [(0, F32(1.0), F32(1.0), F32(0.0))]
    iso = lambda p: np.array([1.0, 0.5, 0.2], np.float32)
    masses, ints = np.array([mass, mass], np.float32), np.array([10.0, 20.0], np.float32)
    g = RI.trace(fmap, [(0, F32(0.5), masses, ints, np.array([1.0, 0.0], np.float32))], al, 1, True, iso)
    g0 = RI.trace(fmap, [(0, F32(0.5), masses, ints, None)], al, 1, True, iso)
    r0 = R.trace(fmap, [(0, F32(0.5), masses, ints)], al, 1, True, iso)
    assert g[(0, 0, False)]["matrix"].sum() == 10.0 and g[(1, 0, False)]["matrix"].sum() == 20.0
    for k in r0:
        assert np.array_equal(g0[k]["matrix"], r0[k]["matrix"]) and g0[k]["matrix"].sum() == 30.0


# ---- the readers ----------------------------------------------------------------------------------------------------------------
def _spectra(rng, with_zero_peaks=False):
    """MS1 with mobility, MS1 without, an MS2 carrying one, MS1 with mobility and a noise array, (an MS1 without peaks)"""
    def peaks(n):
        return np.sort(rng.uniform(300, 1500, n)).astype(np.float32), rng.lognormal(8, 1, n).astype(np.float32)
    sp, levels, mob, noise = [], [], [], []
    for k, (lvl, has_mob, has_noise, n) in enumerate([(1, True, False, 40), (1, False, False, 25), (2, True, False, 30),
                                                      (1, True, True, 35), (1, False, True, 12), (3, True, True, 9)] +
                                                     ([(1, True, False, 0)] if with_zero_peaks else [])):
        mz, it = peaks(n)
        sp.append(RawSpectrum(mz, it, 0.0 if lvl == 1 else 650.25, None if lvl == 1 else 2, None, 1.0 + k, None, 0, f"scan={k + 1}"))
        levels.append(lvl)
        # values that are not exactly representable in f32, so the 64-bit encoding really narrows
        mob.append(rng.uniform(0.6, 1.4, n) if has_mob else None)
        noise.append(rng.uniform(50, 500, n).astype(np.float32) if has_noise else None)
    return sp, levels, mob, noise


def _assert_same(batch, spectra, context):
    assert batch.n == len(spectra), context
    assert (batch.mobility is None) == all(s.mobility is None for s in spectra), context
    for i, s in enumerate(spectra):
        g = batch.spectrum(i)
        assert g.id == s.id, (context, i)
        assert np.array_equal(bits(g.mz), bits(s.mz)) and np.array_equal(bits(g.intensity), bits(s.intensity)), (context, i)
        assert (g.mobility is None) == (s.mobility is None), (context, i)
        if s.mobility is not None:
            assert s.mobility.dtype == np.float32 and np.array_equal(bits(g.mobility), bits(s.mobility)), (context, i)


@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("accession", MOBILITY_ARRAYS)
def test_native_reader_matches_python_reader_with_mobility(tmp_path, accession, width, compress):
    rng = np.random.default_rng(17)
    sp, levels, mob, noise = _spectra(rng)
    p = str(tmp_path / "im.mzML")
    write_mzml(p, sp, levels, noise, mobility=mob, mobility_encoding=(accession, width, compress))
    assert open(p).read().count(f'accession="{accession}"') == sum(m is not None for m in mob)
    for level, sn in ((1, None), (1, 1), (None, 1), (None, None), (2, None), (2, 2), (3, 3)):
        py = read_mzml(p, 0, level, sn)
        _assert_same(read_mzml_native(p, 0, level, sn_level=sn), py, (level, sn))
        # kept at ms level 1 only (spectrum.rs:344), narrowed to f32 element-wise like the other arrays
        for s in py:
            k = int(s.id.split("=")[1]) - 1
            if levels[k] == 1 and mob[k] is not None:
                assert np.array_equal(bits(s.mobility), bits(np.asarray(mob[k], np.float64).astype(np.float32)))
            else:
                assert s.mobility is None
        if level == 1:
            assert [s.id for s in py] == ["scan=1", "scan=2", "scan=4", "scan=5"]
            # a noise array beside the mobility array divides the intensities when S/N is on, and only then
            want = sp[3].intensity / noise[3] if sn == 1 else sp[3].intensity
            assert np.array_equal(bits(py[2].intensity), bits(want))


def test_file_without_mobility_reads_as_before(tmp_path):
    """the optional keyword changes nothing for callers that do not pass it; MS2 output is the same with and without arrays"""
    rng = np.random.default_rng(3)
    sp, levels, mob, noise = _spectra(rng)
    a, b, c = (str(tmp_path / n) for n in ("a.mzML", "b.mzML", "c.mzML"))
    write_mzml(a, sp, levels, noise)
    write_mzml(b, sp, levels, noise, mobility=None)
    write_mzml(c, sp, levels, noise, mobility=mob)
    assert open(a, "rb").read() == open(b, "rb").read() and "mobility" not in open(a).read()
    for level, sn in ((1, None), (1, 1), (2, 2), (None, None)):
        plain = read_mzml_native(a, 0, level, sn_level=sn)
        assert plain.mobility is None and plain.has_mobility is None
        assert all(s.mobility is None for s in read_mzml(a, 0, level, sn))
        withm = read_mzml_native(c, 0, level, sn_level=sn)
        assert plain.ids == withm.ids
        for k in ("peak_off", "mz", "intensities", "precursor_mz", "precursor_charge", "scan_start_time", "file_id"):
            assert np.array_equal(getattr(plain, k), getattr(withm, k)), (level, sn, k)
    assert read_mzml_native(c, 0, 2).mobility is None and read_mzml_native(c, 0, 3).mobility is None


def test_noise_and_mobility_are_kinds_of_their_own(tmp_path):
    """MS:1002744 is noise "only when an array is neither m/z nor intensity"; an ion-mobility accession is the mobility array
    only when the array is none of the three: neither is taken for the other, whatever the order of the cvParams."""
    rng = np.random.default_rng(9)
    sp, levels, mob, noise = _spectra(rng)
    p = str(tmp_path / "x.mzML")
    write_mzml(p, sp[:1], levels[:1], [rng.uniform(50, 500, len(sp[0].mz)).astype(np.float32)], mobility=mob[:1])
    text = open(p).read()
    noise_cv = '<cvParam cvRef="MS" accession="MS:1002744" name="sampled noise intensity array"/>'
    mob_cv = '<cvParam cvRef="MS" accession="MS:1002893" name="ion mobility array"/>'
    assert text.count(noise_cv) == 1 and text.count(mob_cv) == 1
    base = read_mzml(p, 0, 1, 1)[0]
    variants = {
        "mobility term on the m/z array": text.replace('name="m/z array"/>', 'name="m/z array"/>' + mob_cv, 1),
        "mobility term on the intensity array": text.replace('name="intensity array"/>', 'name="intensity array"/>' + mob_cv, 1),
        "mobility term before the intensity term": text.replace('<cvParam cvRef="MS" accession="MS:1000515"',
                                                                mob_cv + '<cvParam cvRef="MS" accession="MS:1000515"', 1),
        "mobility term behind the noise term": text.replace(noise_cv, noise_cv + mob_cv, 1),
        "mobility term before the noise term": text.replace(noise_cv, mob_cv + noise_cv, 1),
    }
    for name, t in variants.items():
        q = str(tmp_path / "v.mzML")
        open(q, "w").write(t)
        for sn in (None, 1):
            py = read_mzml(q, 0, 1, sn)
            _assert_same(read_mzml_native(q, 0, 1, sn_level=sn), py, (name, sn))
            want = read_mzml(p, 0, 1, sn)[0]
            assert np.array_equal(bits(py[0].mz), bits(want.mz)) and np.array_equal(bits(py[0].intensity), bits(want.intensity)), name
            assert np.array_equal(bits(py[0].mobility), bits(base.mobility)), name
    # a noise term on the mobility array: the array is noise, as it reads today, and the spectrum has no mobility
    t = text.replace(mob_cv, mob_cv + noise_cv, 1).replace(noise_cv, "", 1)
    assert t.count(noise_cv) == 1
    open(q, "w").write(t)
    for sn in (None, 1):
        py = read_mzml(q, 0, 1, sn)
        _assert_same(read_mzml_native(q, 0, 1, sn_level=sn), py, ("noise term on the mobility array", sn))
        assert py[0].mobility is None
    assert np.array_equal(bits(read_mzml(q, 0, 1, 1)[0].intensity), bits(sp[0].intensity / np.asarray(mob[0], np.float32)))


def test_mobility_length_mismatch_is_an_error(tmp_path):
    rng = np.random.default_rng(2)
    sp, levels, mob, noise = _spectra(rng)
    mob[0] = mob[0][:-1]
    p = str(tmp_path / "bad.mzML")
    write_mzml(p, sp, levels, mobility=mob)
    with pytest.raises(L.SageHipError, match="ion mobility array of spectrum scan=1 holds 39 values for 40"):
        read_mzml_native(p, 0, 1)
    with pytest.raises(ValueError, match="ion mobility array of spectrum scan=1 holds 39 values for 40"):
        read_mzml(p, 0, 1)
    # the damaged array sits in an MS1 spectrum: a read of another level does not decode it
    assert read_mzml_native(p, 0, 2).n == 1 and len(read_mzml(p, 0, 2)) == 1
    # ... and a short array in an MS2 spectrum is never looked at
    sp, levels, mob, noise = _spectra(rng)
    mob[2] = mob[2][:5]
    write_mzml(p, sp, levels, mobility=mob)
    _assert_same(read_mzml_native(p, 0, None), read_mzml(p, 0, None), "short MS2 array")


def test_spectrum_without_peaks(tmp_path):
    """an MS1 spectrum without peaks and with a mobility array of no values: Some(vec![]) in both readers"""
    rng = np.random.default_rng(4)
    sp, levels, mob, noise = _spectra(rng, with_zero_peaks=True)
    p = str(tmp_path / "e.mzML")
    write_mzml(p, sp, levels, mobility=mob)
    py = read_mzml(p, 0, 1)
    _assert_same(read_mzml_native(p, 0, 1), py, "empty")
    assert py[-1].id == "scan=7" and len(py[-1].mz) == 0 and py[-1].mobility is not None and len(py[-1].mobility) == 0


# ---- batches --------------------------------------------------------------------------------------------------------------------
def test_raw_batch_carries_the_column():
    rng = np.random.default_rng(6)
    sp, levels, mob, _ = _spectra(rng)
    ms1 = [RawSpectrum(s.mz, s.intensity, 0.0, None, None, s.scan_start_time, None, 0, s.id,
                       mobility=None if m is None else m.astype(np.float32)) for s, l, m in zip(sp, levels, mob) if l == 1]
    b = RawBatch(ms1)
    assert b.has_mobility.tolist() == [1, 0, 1, 0] and len(b.mobility) == len(b.mz)
    assert not b.mobility[int(b.peak_off[1]):int(b.peak_off[2])].any()
    for view in (b, b.slice(1, 4), b.subset([3, 2, 0]), b.subset([1, 3])):
        idx = {s.id: s for s in ms1}
        for i in range(view.n):
            g = view.spectrum(i)
            want = idx[g.id]
            assert (g.mobility is None) == (want.mobility is None)
            if want.mobility is not None:
                assert np.array_equal(bits(g.mobility), bits(want.mobility))
    assert RawBatch([s for s in ms1 if s.mobility is None]).mobility is None
    with pytest.raises(ValueError):
        RawBatch([RawSpectrum(sp[0].mz, sp[0].intensity, 0.0, mobility=np.zeros(3, np.float32))])


def test_header_declares_the_entry_points():
    import os
    hdr = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "sage_hip.h")).read()
    for name in ("sage_hip_lfq_im", "sage_hip_mzml_mobility", "sage_hip_mzml_has_mobility"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.EXPORTED_SYMBOLS and hasattr(L.load(), name)
    assert C.sizeof(L.SageLfqMobility) == 16
