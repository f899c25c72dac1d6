"""TMT quantification without a GPU: the `quant.tmt` section of the JSON config, the reporter tables, the level-2 cut-off,
the mzML fields TMT reads (C++ reader against its Python twin, signal-to-noise included) and the tmt.tsv writer against its
Python twin."""
import os

import numpy as np
import pytest

import tmt_reference as R
from sage_amd import output
from sage_amd.api import Isobaric, RawSpectrum, TmtSettings
from sage_amd.cli import tmt_settings
from sage_amd.mzml import read_mzml, read_mzml_native, write_mzml


def test_reference_self_test():
    assert R.self_test()


def test_tmt_settings_defaults_and_variants():
    logs = []
    iso, st = tmt_settings({}, logs.append)
    assert iso is None and st == TmtSettings(3, False) and logs == []
    iso, st = tmt_settings({"quant": {"lfq": True}}, logs.append)
    assert iso is None and st.level == 3 and not st.sn
    for v, n in (("Tmt6", 6), ("Tmt10", 10), ("Tmt11", 11), ("Tmt16", 16), ("Tmt18", 18)):
        iso, st = tmt_settings({"quant": {"tmt": v}}, logs.append)
        assert iso.kind == v and len(iso.reporter_masses()) == n and iso.headers() == [f"tmt_{i}" for i in range(1, n + 1)]
    iso, st = tmt_settings({"quant": {"tmt": {"User": [131.0, 126.5, 126.5]}, "tmt_settings": {"level": 2, "sn": True}}}, logs.append)
    assert iso.kind == "User" and iso.headers() == ["user_1", "user_2", "user_3"] and st == TmtSettings(2, True)
    assert iso.reporter_masses().dtype == np.float32 and list(iso.reporter_masses()) == [np.float32(131.0), np.float32(126.5)] * 1 + [np.float32(126.5)]
    iso, _ = tmt_settings({"quant": {"tmt": {"User": []}}}, logs.append)
    assert iso.headers() == [] and len(iso.reporter_masses()) == 0 and iso.modification_mass() is None
    assert logs == []


def test_tmt_settings_unknown_variant_and_level_warning():
    with pytest.raises(SystemExit, match="`Tmt7`"):
        tmt_settings({"quant": {"tmt": "Tmt7"}})
    with pytest.raises(SystemExit, match="`Itraq4`"):
        tmt_settings({"quant": {"tmt": {"Itraq4": [1.0]}}})
    for level in (1, 4):
        logs = []
        tmt_settings({"quant": {"tmt": "Tmt6", "tmt_settings": {"level": level}}}, logs.append)
        assert logs == [f"TMT quant level set at {level}, is this correct?"]
    logs = []
    tmt_settings({"quant": {"tmt": "Tmt6", "tmt_settings": {"level": 2}}}, logs.append)
    assert logs == []


def test_reporter_tables():
    t18 = Isobaric("Tmt18").reporter_masses()
    assert t18[0] == np.float32(126.127726) and t18[-1] == np.float32(135.15160) and t18[10] == np.float32(131.144500)
    assert Isobaric("Tmt11").reporter_masses()[10] == np.float32(131.144499)
    assert np.array_equal(Isobaric("Tmt16").reporter_masses(), t18[:16])
    assert np.array_equal(Isobaric("Tmt10").reporter_masses(), Isobaric("Tmt11").reporter_masses()[:10])
    assert list(Isobaric("Tmt6").reporter_masses()) == [np.float32(x) for x in
                                                       (126.127726, 127.124761, 128.134436, 129.131471, 130.141145, 131.138180)]
    assert Isobaric("Tmt6").modification_mass() == 229.162932 and Isobaric("Tmt18").modification_mass() == 304.2135
    assert Isobaric("Tmt16").modification_mass() == 304.2071


def test_min_deisotope_cutoff_is_f32_of_last_label():
    for iso in (Isobaric("Tmt16"), Isobaric("Tmt18"), Isobaric("User", (140.0, 120.0))):
        m = iso.reporter_masses()
        want = np.float32(m[-1] * np.float32(np.float32(1.0) + np.float32(20e-6)))
        assert np.float32(iso.min_deisotope_mz()) == want == R.min_deisotope_mz(m)
    assert Isobaric("User", (140.0, 120.0)).min_deisotope_mz() < 121.0  # last, not max
    assert Isobaric("User", ()).min_deisotope_mz() == 0.0


def _spectrum(i, level, n, rng, ref="", iit=0.0):
    mz = np.sort(rng.uniform(100.0, 140.0, n)).astype(np.float32)
    return RawSpectrum(mz, rng.uniform(0.0, 1e5, n).astype(np.float32), 500.0 if level > 1 else 0.0, 2 if level > 1 else None,
                       scan_start_time=float(i), id=f"s {i}", ion_injection_time=iit, precursor_ref=ref)


def test_reader_fields_and_signal_to_noise(tmp_path):
    rng = np.random.default_rng(1)
    spectra, levels, noise = [], [], []
    # MS2 with injection time; MS3 with a ref and its own noise; MS3 with a SHORTER noise array; MS3 with noise zeros;
    # MS3 without noise (after one whose noise went unused at another level); MS2 with a noise array (not the S/N level)
    spectra.append(_spectrum(0, 2, 8, rng, iit=12.5)); levels.append(2); noise.append(rng.uniform(1, 9, 8).astype(np.float32))
    spectra.append(_spectrum(1, 3, 10, rng, ref="s 0", iit=33.25)); levels.append(3); noise.append(rng.uniform(1, 9, 10).astype(np.float32))
    spectra.append(_spectrum(2, 3, 10, rng, ref="s 0")); levels.append(3); noise.append(rng.uniform(1, 9, 4).astype(np.float32))
    z = np.zeros(6, np.float32)
    s3 = _spectrum(3, 3, 6, rng, ref="a&b")
    s3.intensity[0] = 0.0
    spectra.append(s3); levels.append(3); noise.append(z)
    spectra.append(_spectrum(4, 1, 5, rng)); levels.append(1); noise.append(rng.uniform(1, 9, 5).astype(np.float32))
    spectra.append(_spectrum(5, 3, 7, rng)); levels.append(3); noise.append(None)
    path = str(tmp_path / "sn.mzML")
    write_mzml(path, spectra, levels, noise, [None, [130.0, 131.0], None, None, None, None])
    for ms_level in (None, 2, 3):
        for sn in (None, 2, 3):
            py = read_mzml(path, 0, ms_level, sn)
            nat = read_mzml_native(path, 0, ms_level, sn_level=sn)
            assert nat.n == len(py)
            for i, p in enumerate(py):
                q = nat.spectrum(i)
                assert q.id == p.id and q.precursor_ref == p.precursor_ref
                assert np.float32(q.ion_injection_time) == np.float32(p.ion_injection_time)
                assert np.array_equal(q.mz, p.mz)
                assert np.array_equal(q.intensity.view(np.uint32), np.asarray(p.intensity, np.float32).view(np.uint32))
    ms3 = read_mzml_native(path, 0, 3, sn_level=3)
    base = read_mzml_native(path, 0, 3)
    assert list(ms3.precursor_ref) == ["s 0", "s 0", "a&b", ""]
    assert list(read_mzml_native(path, 0, 2).ion_injection_time) == [np.float32(12.5)]
    assert ms3.ion_injection_time[0] == np.float32(33.25) and ms3.ion_injection_time[1] == 0.0
    for k, src in enumerate((1, 2, 3, 5)):
        got = ms3.intensities[int(ms3.peak_off[k]):int(ms3.peak_off[k + 1])]
        want = R.signal_to_noise(spectra[src].intensity, noise[src])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
    # noise 0: x / 0 -> inf, 0 / 0 -> NaN; the spectrum without a noise array keeps its intensities (no carry-over)
    s3_got = ms3.intensities[int(ms3.peak_off[2]):int(ms3.peak_off[3])]
    assert np.isnan(s3_got[0]) and np.all(np.isinf(s3_got[1:]))
    assert np.array_equal(ms3.intensities[int(ms3.peak_off[3]):], spectra[5].intensity)
    # the shorter noise array divides only its length
    short = ms3.intensities[int(ms3.peak_off[1]):int(ms3.peak_off[2])]
    assert np.array_equal(short[4:], spectra[2].intensity[4:])
    # without S/N, or at another level, nothing changes
    assert np.array_equal(base.intensities, np.concatenate([spectra[i].intensity for i in (1, 2, 3, 5)]))
    assert np.array_equal(read_mzml_native(path, 0, 2, sn_level=3).intensities, spectra[0].intensity)


def test_reader_without_sn_is_unchanged(tmp_path):
    """write_mzml's default output and read_mzml_native without the new argument: no noise division, ids as before."""
    rng = np.random.default_rng(2)
    spectra = [_spectrum(i, 2, 12, rng) for i in range(5)]
    path = str(tmp_path / "plain.mzML")
    write_mzml(path, spectra)
    text = open(path).read()
    assert "MS:1000927" not in text and "spectrumRef" not in text and "MS:1002744" not in text
    b = read_mzml_native(path)
    assert b.n == 5 and np.array_equal(b.intensities, np.concatenate([s.intensity for s in spectra]))
    assert list(b.precursor_ref) == [""] * 5 and np.all(b.ion_injection_time == 0.0)


def test_write_tmt_native_matches_python_twin(tmp_path):
    vals = np.array([[-0.0, np.inf, np.nan], [1e-7, 3e38, 0.0], [126.5, 1.0, 123456.789]], dtype=np.float32)
    headers = ["tmt_1", "tmt_2", "tmt_3"]
    names = ["a.mzML", "b c.mzML"]
    fid = [0, 1, 1]
    ids = ["controllerType=0 controllerNumber=1 scan=7", "", "scan=9"]
    iit = np.array([12.5, 0.0, 1e-7], dtype=np.float32)
    p1, p2 = str(tmp_path / "native.tsv"), str(tmp_path / "py.tsv")
    output.write_tmt_native(p1, headers, names, fid, ids, iit, vals)
    output.write_tmt(p2, headers, output.tmt_rows(names, fid, ids, iit, vals))
    a, b = open(p1, "rb").read(), open(p2, "rb").read()
    assert a == b
    lines = a.decode().split("\n")
    assert lines[0] == "filename\tscannr\tion_injection_time\ttmt_1\ttmt_2\ttmt_3"
    assert lines[1] == "a.mzML\tcontrollerType=0 controllerNumber=1 scan=7\t12.5\t-0.0\tinf\tNaN"
    assert lines[2] == "b c.mzML\t\t0.0\t1e-7\t3e38\t0.0"
    # no labels: the three leading columns only
    output.write_tmt_native(p1, [], names, fid, ids, iit, np.zeros((3, 0), np.float32))
    output.write_tmt(p2, [], output.tmt_rows(names, fid, ids, iit, np.zeros((3, 0), np.float32)))
    assert open(p1, "rb").read() == open(p2, "rb").read()
    assert open(p1).read().split("\n")[1] == "a.mzML\tcontrollerType=0 controllerNumber=1 scan=7\t12.5"


def test_sps_generator_round_trip(tmp_path):
    from sage_amd.api import DatabaseParameters
    from sage_amd.lcms import synthetic_sps_ms3, write_sps
    from sage_amd.synthetic import synthetic_fasta
    db = DatabaseParameters(enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P")).build(synthetic_fasta(40, seed=3))
    files = synthetic_sps_ms3(db, Isobaric("Tmt18").reporter_masses(), n_files=1, ms2_per_file=12, seed=4)
    assert files[0].ms_levels.count(3) == 12 and files[0].ms_levels.count(2) == 12
    paths = write_sps(str(tmp_path), files)
    ms3 = read_mzml_native(paths[0], 0, 3, sn_level=3)
    ms2 = read_mzml_native(paths[0], 0, 2)
    assert ms3.n == 12 and list(ms3.precursor_ref) == list(ms2.ids)
    assert np.all(ms3.ion_injection_time > 0) and np.all(ms2.ion_injection_time > 0)
    py = read_mzml(paths[0], 0, 3, 3)
    assert np.array_equal(np.concatenate([p.intensity for p in py]).view(np.uint32), ms3.intensities.view(np.uint32))
