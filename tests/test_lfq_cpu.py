"""Label-free quantification without a GPU: the restatement (tests/lfq_reference.py) pinned to what the reference itself
asserts, the `quant` section of the JSON config, the lfq.tsv writer against its Python twin, the mzML MS1 round trip."""
import math
import os

import numpy as np
import pytest

import lfq_reference as R
from sage_amd import output
from sage_amd.api import LfqResult, LfqSettings, peptide_compositions
from sage_amd.cli import quant_settings


def test_peptide_isotopes_smoke_vector():
    # isotopes.rs:57-67
    iso = R.peptide_isotopes(60, 5)
    expected = np.array([0.3972, 0.2824, 0.1869]) / 0.3972
    assert iso.dtype == np.float32
    assert np.all(np.abs(iso.astype(np.float64) - expected) <= 0.02), iso


def test_binary_search_slice_reference_cases():
    # database.rs:570-600
    data = [1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
    assert R.binary_search_slice(data, 1.75, 3.5) == (1, 6)
    assert R.binary_search_slice(data, 0.0, 5.0) == (0, len(data))
    data = [1.0, 1.5, 1.5, 1.5, 1.5, 2.0, 2.5, 3.0, 3.0, 3.5, 4.0]
    left, right = R.binary_search_slice(data, 1.5, 3.25)
    assert data[left] <= 1.5 and data[right] > 3.25
    assert data[left:right] == [1.0, 1.5, 1.5, 1.5, 1.5, 2.0, 2.5, 3.0, 3.0]
    assert R.binary_search_slice([], 1.0, 2.0) == (0, 0)


def test_convolve_against_numpy_where_they_agree():
    """lfq.rs:611 says convolve behaves like np.convolve(.., mode='same').  That holds for an odd-length symmetric kernel;
    for the even K_WIDTH = 10 kernel it holds from bin 5 on (where the whole kernel fits on the left), one bin to the right
    of np.convolve's 'same' window; the first five bins use a different part of the kernel."""
    rng = np.random.default_rng(3)
    x = rng.random(100)
    odd = R.gaussian_kernel(0.5, 9)
    np.testing.assert_allclose(R.convolve(x, odd)[0], np.convolve(x, odd, mode="same"), rtol=1e-12, atol=1e-15)
    k = R.gaussian_kernel(0.5, R.K_WIDTH)
    full = np.convolve(x, k, mode="full")
    np.testing.assert_allclose(R.convolve(x, k)[0][5:], full[10:105], rtol=1e-12, atol=1e-15)
    assert not np.allclose(R.convolve(x, k)[0][:5], full[5:10])
    assert abs(sum(k) - 1.0) < 1e-15 and np.allclose(k, k[::-1], rtol=1e-15)


def test_convolve_is_the_sequential_loop():
    x = np.arange(1.0, 101.0)
    k = R.gaussian_kernel(0.5, R.K_WIDTH)
    out = R.convolve(x, k)[0]
    for idx in (0, 3, 4, 5, 50, 95, 99):
        kk = k[max(len(k) - (5 + idx), 0):]
        w = x[max(idx - 4, 0):]
        acc = 0.0
        for a, b in zip(w, kk):
            acc = acc + a * b
        assert out[idx] == acc


def test_picked_precursor_ties_and_counts():
    rows = [((1, 0, False), 3.0), ((1, 0, True), 1.0), ((2, 0, False), 2.0), ((3, 0, False), 2.0), ((3, 0, True), 2.0)]
    q, passing = R.picked_precursor(rows)
    # order: 3.0 (T), 2.0 (T pep 2), 2.0 (T pep 3), 2.0 (D pep 3), 1.0 (D); decoy / target = 1, 1/2, 1/3, 2/3, 1
    third = np.float32(1.0) / np.float32(3.0)
    assert q[(1, 0, False)] == third and q[(2, 0, False)] == third and q[(3, 0, False)] == third
    assert q[(3, 0, True)] == np.float32(2.0) / np.float32(3.0)
    assert q[(1, 0, True)] == np.float32(1.0)
    assert passing == 0


def test_quant_settings_defaults_and_absent_keys():
    on, st = quant_settings({}, log=lambda m: None)
    assert on is False and st == LfqSettings()
    on, st = quant_settings({"quant": {}}, log=lambda m: None)
    assert on is False and st == LfqSettings()
    on, st = quant_settings({"quant": {"lfq": True}}, log=lambda m: None)
    assert on is True and st == LfqSettings(peak_scoring="Hybrid", integration="Sum", spectral_angle=0.70, ppm_tolerance=5.0,
                                            mobility_pct_tolerance=1.0, combine_charge_states=True, peptide_q_value=0.01)


def test_quant_settings_values_enums_and_warnings():
    msgs = []
    on, st = quant_settings({"quant": {"lfq": True, "lfq_settings": {
        "peak_scoring": "SpectralAngle", "integration": "Apex", "spectral_angle": -0.4, "ppm_tolerance": -25.0,
        "combine_charge_states": False, "peptide_q_value": 0.05, "mobility_pct_tolerance": 5.0}}}, log=msgs.append)
    assert on and st.peak_scoring == "SpectralAngle" and st.integration == "Apex"
    assert st.spectral_angle == 0.4 and st.ppm_tolerance == 25.0 and st.combine_charge_states is False
    assert "lfq_settings.ppm_tolerance is higher than expected" in msgs
    assert "lfq_settings.spectral_angle is lower than expected" in msgs
    assert "lfq_settings.mobility_pct_tolerance is higher than expected" in msgs
    assert any(m.startswith("lfq_settings.peptide_q_value is higher") for m in msgs)
    for v in ("RetentionTime", "Intensity", "Hybrid"):
        assert quant_settings({"quant": {"lfq_settings": {"peak_scoring": v}}}, log=lambda m: None)[1].peak_scoring == v
    with pytest.raises(SystemExit):
        quant_settings({"quant": {"lfq_settings": {"peak_scoring": "hybrid"}}}, log=lambda m: None)
    with pytest.raises(SystemExit):
        quant_settings({"quant": {"lfq_settings": {"integration": "Area"}}}, log=lambda m: None)


def test_peptide_compositions():
    seqs = ["PEPTIDE", "CMK", ""]
    off = np.cumsum([0] + [len(s) for s in seqs])
    c, s = peptide_compositions(off, np.frombuffer("".join(seqs).encode(), np.uint8))
    for i, q in enumerate(seqs):
        assert (int(c[i]), int(s[i])) == R.composition(q)


def _fixed_result(n_files=3):
    rng = np.random.default_rng(1)
    n = 6
    areas = rng.lognormal(12, 2, (n, n_files))
    areas[0, 1] = 0.0
    areas[2, 0] = 1e-310
    return LfqResult(np.array([0, 0, 1, 2, 2, 3], np.uint32), np.array([0, 0, 2, 3, 3, 0], np.uint8),
                     np.array([0, 1, 0, 0, 1, 0], np.uint8), np.array([1, 1, 1, 1, 1, 0], np.uint8), np.zeros(n, np.uint32),
                     np.zeros(n, np.uint32), np.zeros(n, np.uint32), rng.random(n) * 3, np.array([0.9, 0.8, 1.0, 0.71, 0.5, 0.0]),
                     np.array([0.0, 1.0, 0.012345679, 0.05, 1.0, 1.0], np.float32), areas, np.zeros((n, n_files), np.int32), None,
                     0, 0, 0, {})


def test_lfq_writer_native_matches_python_twin(tmp_path):
    from sage_amd.api import DatabaseParameters
    from sage_amd.synthetic import synthetic_fasta
    db = DatabaseParameters(enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                            static_mods={"C": 57.0215}, variable_mods={"M": [15.9949]}).build(synthetic_fasta(5, seed=2))
    res = _fixed_result()
    names = ["a.mzML", "b.mzML.gz", "c"]
    rows = res.target_rows()
    assert rows.tolist() == [0, 2, 3]  # targets with a peak, grid order
    native, twin = tmp_path / "native.tsv", tmp_path / "twin.tsv"
    output.write_lfq_native(str(native), db, res, names)
    output.write_lfq(str(twin), names, output.lfq_rows(db, res, rows))
    assert native.read_bytes() == twin.read_bytes()
    lines = native.read_text().splitlines()
    assert lines[0] == "peptide\tcharge\tproteins\tq_value\tscore\tspectral_angle\ta.mzML\tb.mzML.gz\tc"
    assert lines[1].split("\t")[1] == "-1" and lines[2].split("\t")[1] == "2"
    assert lines[1].split("\t")[3] == "0.0" and lines[2].split("\t")[3] == "0.012345679"
    assert lines[1].split("\t")[7] == "0.0" and lines[2].split("\t")[6] == "1e-310"


def test_mzml_ms1_round_trip(tmp_path):
    from sage_amd.api import DatabaseParameters
    from sage_amd.lcms import synthetic_lcms, write_lcms
    from sage_amd.mzml import read_mzml, read_mzml_native
    from sage_amd.synthetic import synthetic_fasta
    db = DatabaseParameters(enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P")).build(synthetic_fasta(20, seed=4))
    files = synthetic_lcms(db, n_files=2, n_peptides=8, ms1_per_file=30, seed=5)
    paths = write_lcms(str(tmp_path), files)
    for f, p in enumerate(paths):
        lvl = np.array(files[f].ms_levels)
        ms1 = read_mzml_native(p, f, 1)
        ms2 = read_mzml_native(p, f, 2, check_searchable=True)
        assert ms1.n == (lvl == 1).sum() and ms2.n == (lvl == 2).sum()
        py = read_mzml(p, f, 1)
        want = [s for s, l in zip(files[f].spectra, lvl) if l == 1]
        for i, s in enumerate(want):
            a, b = int(ms1.peak_off[i]), int(ms1.peak_off[i + 1])
            np.testing.assert_array_equal(ms1.mz[a:b], s.mz)
            np.testing.assert_array_equal(py[i].intensity, s.intensity)
            assert ms1.scan_start_time[i] == np.float32(s.scan_start_time) and ms1.file_id[i] == f
        assert np.all(np.diff(ms1.scan_start_time) >= 0)


def test_process_ms1_keeps_every_peak_stably_sorted():
    mz = np.array([500.0, 400.0, 400.0, 300.0], np.float32)
    it = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    m, i = R.process_ms1(mz, it)
    assert m.tolist() == (np.array([300.0, 400.0, 400.0, 500.0], np.float32) - R.PROTON).tolist()
    assert i.tolist() == [4.0, 2.0, 3.0, 1.0]


def test_add_entry_saturating_bins():
    g = dict(rt_min=np.float32(0.5) - R.RT_TOL, rt_step=(R.RT_TOL * np.float32(2.0)) / np.float32(100),
             matrix=np.zeros((3, 100)))
    below = np.nextafter(g["rt_min"], np.float32(0))  # floor(...) = -1 -> bin 0, interp < 0
    R.add_entry(g, below, 0, 0, np.float32(10.0))
    assert g["matrix"][0, 0] > 10.0 and g["matrix"][0, 1] < 0.0
    R.add_entry(g, np.float32(0.5) + R.RT_TOL, 1, 0, np.float32(10.0))  # bin 100 -> 99, both halves into bin 99
    assert g["matrix"][1, 99] != 0.0 and g["matrix"][1, :99].sum() == 0.0
    assert math.isclose(g["matrix"][1, 99], 10.0, rel_tol=1e-5)
