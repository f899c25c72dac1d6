"""MGF input without a GPU: the C++ reader (csrc/mgf_reader.cpp) against the sequential restatement tests/mgf_reference.py, on a
fixture and on randomised texts that exercise every quirk of mgf.rs; piece cutting; the f32 grammar; errors; the extension
dispatch; the CSV quoting of the writers."""
import gzip
import os
import random

import numpy as np
import pytest

import mgf_reference as R
from sage_amd import _lib as L
from sage_amd.api import RawSpectrum
from sage_amd.mgf import TOL_DA, is_mgf, parse_f32, read_mgf_native, read_spectra, write_mgf

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def assert_same(path, text, file_id=3):
    want, _ = R.read_mgf(text, file_id)
    b, kinds, zero = read_mgf_native(path, file_id=file_id)
    assert b.n == len(want)
    assert b.ids == [s["id"] for s in want]
    np.testing.assert_array_equal(bits(b.precursor_mz), bits([s["precursor_mz"] for s in want]))
    np.testing.assert_array_equal(b.precursor_charge, [s["charge"] or 0 for s in want])
    np.testing.assert_array_equal(zero, [int(s["charge"] == 0) for s in want])
    np.testing.assert_array_equal(bits(b.scan_start_time), bits([s["scan_start_time"] for s in want]))
    np.testing.assert_array_equal(b.file_id, [file_id] * len(want))
    # (a window of TOL=NaN, which matches nothing, is carried as the empty window (+inf, -inf): sage_hip_mgf_read)
    iso = [w if w is None or not np.isnan(w[2]) else (w[0], np.float32(np.inf), np.float32(-np.inf)) for w in (s["isolation"] for s in want)]
    none = [w is None for w in iso]
    np.testing.assert_array_equal(np.isnan(b.isolation_lo), none)
    np.testing.assert_array_equal(np.isnan(b.isolation_hi), none)
    has = ~np.array(none, bool)
    np.testing.assert_array_equal(bits(b.isolation_lo[has]), bits([w[1] for w in iso if w]))
    np.testing.assert_array_equal(bits(b.isolation_hi[has]), bits([w[2] for w in iso if w]))
    np.testing.assert_array_equal(kinds, [w[0] if w else TOL_DA for w in iso])
    assert np.isnan(b.inverse_ion_mobility).all() and (b.ion_injection_time == 0).all()
    off = np.concatenate([[0], np.cumsum([len(s["mz"]) for s in want])]).astype(np.uint64)
    np.testing.assert_array_equal(b.peak_off, off)
    cat = lambda k: np.concatenate([s[k] for s in want]) if want else np.zeros(0, np.float32)
    np.testing.assert_array_equal(bits(b.mz), bits(cat("mz")))
    np.testing.assert_array_equal(bits(b.intensities), bits(cat("intensity")))
    return b


def test_fixture_quirks(tmp_path):
    path = os.path.join(GOLDEN, "mgf_quirks.mgf")
    text = open(path, encoding="utf-8").read()
    b = assert_same(path, text)
    spectra, dropped = R.read_mgf(text)
    # the defaults skip spectrum 1 and apply to the second (whose PEPMASS came before its BEGIN IONS)
    assert spectra[0]["isolation"] is None and spectra[0]["charge"] is None
    assert spectra[1]["charge"] == 3 and spectra[1]["isolation"][0] == R.TOL_PPM and spectra[1]["precursor_mz"] == np.float32(505.7701)
    assert [s["charge"] for s in spectra[2:5]] == [2, 1, 0]
    assert len(dropped) == 2 and b.n == 6
    gz = tmp_path / "quirks.mgf.gz"
    gz.write_bytes(gzip.compress(text.encode()))
    assert_same(str(gz), text)


def _num(rng):
    r = rng.random()
    if r < 0.6:
        return f"{rng.uniform(0, 2000):.{rng.randint(0, 7)}f}"
    return rng.choice(["1e3", "+12.5", "-4", ".5", "5.", "1E-2", "inf", "NaN", "-Infinity", "0x10", "1e", "", "abc", "nan(1)",
                       "1_0", "12,5", "3.4028236e38", "1e-46", "7.006e-46", "00012.50", "+", "-.", "١٢"])


def _line(rng):
    r = rng.random()
    if r < 0.45:  # peaks
        k = rng.random()
        if k < 0.7:
            return f"{rng.uniform(100, 2000):.4f} {rng.uniform(0, 1e5):.2f}"
        if k < 0.8:
            return f"{rng.uniform(100, 2000):.3f}"
        if k < 0.9:
            return f"{rng.uniform(100, 2000):.3f}\t{_num(rng)}\textra"
        return rng.choice(["12abc 5", "1 x", ".5 3", "-2 3", "9 9 9 9", "3e2 1e1"])
    if r < 0.55:
        return "PEPMASS=" + " ".join(_num(rng) for _ in range(rng.randint(0, 3)))
    if r < 0.63:
        return "CHARGE=" + rng.choice(["2+", "3", "2+ and 3+", "10+", "+", "0", "", "4-", "٣+", "1+2+3+"])
    if r < 0.70:
        return "TOL=" + _num(rng)
    if r < 0.76:
        return "TOLU=" + rng.choice(["ppm", "Da", "da", "PPM", "mmu", "", "ppm "])
    if r < 0.82:
        return "RTINSECONDS=" + rng.choice([_num(rng), "60-62", f"{rng.uniform(0, 7200):.3f}"])
    if r < 0.88:
        return "TITLE=" + rng.choice(["", "a b", 'q"uoted"', "scan=7", "ü x", f"index={rng.randint(0, 99)}"])
    return rng.choice(["", "   ", "COM=x", "BEGIN IONS", "SCANS=3", " END IONS", "END IONSx", "END IONS", "\x0b5 5"])


def random_mgf(rng):
    out = []
    for _ in range(rng.randint(0, 3)):
        out.append(rng.choice(["TOL=10", "TOLU=ppm", "TOLU=Da", "CHARGE=2+", "CHARGE=0", "TOL=0.5", "COM=header"]))
    out.append(rng.choice(["BEGIN IONS", "  BEGIN IONS", "BEGIN IONS trailing"]))
    for _ in range(rng.randint(0, 8)):
        body = [f"TITLE=s{rng.randint(0, 999)}", f"PEPMASS={rng.uniform(300, 1500):.4f}"] if rng.random() < 0.7 else []
        body += [_line(rng) for _ in range(rng.randint(0, 10))]
        rng.shuffle(body)
        out += body + [rng.choice(["END IONS", "END IONS", " END IONS "])]
        if rng.random() < 0.3:
            out.append(_line(rng))
        out.append("BEGIN IONS")
    nl = rng.choice(["\n", "\r\n"])
    return nl.join(out) + (nl if rng.random() < 0.8 else "")


def test_random_texts_match_reference(tmp_path):
    rng = random.Random(20261016)
    for k in range(200):
        text = random_mgf(rng)
        name = tmp_path / (f"r{k}.mgf.gz" if k % 7 == 0 else f"r{k}.mgf")
        data = text.encode()
        name.write_bytes(gzip.compress(data) if k % 7 == 0 else data)
        assert_same(str(name), text)


def test_pieces_give_the_same_result(tmp_path, monkeypatch):
    rng = random.Random(7)
    text = "TOL=5\nTOLU=ppm\nCHARGE=2\nBEGIN IONS\n" + "".join(random_mgf(rng).split("BEGIN IONS", 1)[1] for _ in range(300))
    path = tmp_path / "big.mgf"
    path.write_text(text, encoding="utf-8")
    monkeypatch.delenv("SAGE_HIP_MGF_PIECE_KB", raising=False)
    whole = assert_same(str(path), text)
    monkeypatch.setenv("SAGE_HIP_MGF_PIECE_KB", "1")
    small = assert_same(str(path), text)
    assert whole.n == small.n and whole.n > 100 and len(text) > 16 * 1024


F32_TABLE = [  # token, accepted, value
    ("1", True, 1.0), ("+1.5", True, 1.5), ("-2", True, -2.0), (".5", True, 0.5), ("5.", True, 5.0), ("1e3", True, 1000.0),
    ("1E+3", True, 1000.0), ("2.5e-1", True, 0.25), ("inf", True, np.inf), ("-Infinity", True, -np.inf), ("INF", True, np.inf),
    ("NaN", True, np.nan), ("0.1", True, np.float32(0.1)), ("3.4028235e38", True, np.float32(3.4028235e38)),
    ("3.40282355e38", True, np.float32(3.4028235e38)), ("3.4028236e38", True, np.inf), ("3.5e38", True, np.inf), ("1e-46", True, 0.0),
    ("1.4e-45", True, np.float32(1.4e-45)), ("16777217", True, 16777216.0), ("16777219", True, 16777220.0),
    ("0.30000001192092896", True, np.float32(0.3)), ("000123.4500", True, np.float32(123.45)),
    ("", False, None), ("+", False, None), (".", False, None), ("e5", False, None), ("1e", False, None), ("1e+", False, None),
    ("0x10", False, None), (" 1", False, None), ("1 ", False, None), ("nan(1)", False, None), ("infin", False, None),
    ("1_000", False, None), ("1,5", False, None), ("--1", False, None), ("١", False, None), ("1.2.3", False, None),
]


@pytest.mark.parametrize("token,ok,value", F32_TABLE)
def test_f32_grammar(token, ok, value):
    ref = R.rust_f32(token)
    got = parse_f32(token)
    assert (ref is not None) == ok and (got is not None) == ok
    if ok:
        if np.isnan(value):
            assert np.isnan(ref) and np.isnan(got)
        else:
            assert bits(ref) == bits(np.float32(value)) == bits(np.float32(got))


def test_f32_random_decimal_rounding():
    rng = random.Random(3)
    for _ in range(3000):
        tok = f"{rng.randint(0, 10 ** rng.randint(1, 12))}.{rng.randint(0, 10 ** 9):09d}e{rng.randint(-50, 40)}"
        assert bits(R.rust_f32(tok)) == bits(np.float32(parse_f32(tok))), tok


def test_errors_are_statuses(tmp_path):
    p = tmp_path / "no_begin.mgf"
    p.write_text("TOL=10\nTITLE=x\n100 1\nEND IONS\n")
    with pytest.raises(ValueError):
        R.read_mgf(p.read_text())
    with pytest.raises(L.SageHipError, match="BEGIN IONS"):
        read_mgf_native(str(p))
    with pytest.raises(L.SageHipError, match="cannot open"):
        read_mgf_native(str(tmp_path / "missing.mgf"))
    bad = tmp_path / "bad_utf8.mgf"
    bad.write_bytes(b"BEGIN IONS\nTITLE=\xff\nPEPMASS=1\n1 1\nEND IONS\n")
    with pytest.raises(L.SageHipError, match="UTF-8"):
        read_mgf_native(str(bad))
    empty = tmp_path / "only_begin.mgf"
    empty.write_text("BEGIN IONS")
    b, kinds, zero = read_mgf_native(str(empty))
    assert b.n == 0 and len(kinds) == 0 and len(zero) == 0


def test_extension_dispatch(tmp_path):
    for p, want in (("a.mgf", True), ("A.MGF", True), ("x/b.Mgf.Gz", True), ("c.mzML", False), ("c.mzml.gz", False),
                    ("d.mgf.bak", False), ("e.gz", False), ("mgf", False)):
        assert is_mgf(p) == want and (R.file_format(p) == "mgf") == want
    s = [RawSpectrum(np.array([100.5, 200.25], np.float32), np.array([3.0, 4.0], np.float32), 500.25, 2, (-1.5, 1.5),
                     np.float32(12.0) / np.float32(60.0), id="controllerType=0 scan=1")]
    from sage_amd.mzml import write_mzml
    write_mgf(str(tmp_path / "s.MGF"), s)
    write_mzml(str(tmp_path / "s.mzML"), s)
    a, ka, za = read_spectra(str(tmp_path / "s.MGF"))
    m, km, zm = read_spectra(str(tmp_path / "s.mzML"))
    for k in ("peak_off", "mz", "intensities", "precursor_mz", "precursor_charge", "isolation_lo", "isolation_hi", "scan_start_time"):
        np.testing.assert_array_equal(getattr(a, k), getattr(m, k), err_msg=k)
    assert a.ids == m.ids and list(ka) == list(km) == [TOL_DA] and list(za) == list(zm) == [0]
    # MGF holds MS2 only: other levels read nothing; sn is not an MGF option
    assert read_spectra(str(tmp_path / "s.MGF"), ms_level=1)[0].n == 0
    assert read_spectra(str(tmp_path / "s.MGF"), ms_level=2, sn_level=2)[0].n == 1


def test_write_mgf_round_trip_ppm_and_crlf(tmp_path):
    rng = np.random.default_rng(5)
    spectra = []
    for i in range(20):
        n = int(rng.integers(1, 30))
        secs = np.float32(rng.uniform(0, 5000))
        spectra.append(RawSpectrum(np.sort(rng.uniform(100, 2000, n)).astype(np.float32), rng.uniform(1, 1e6, n).astype(np.float32),
                                   float(np.float32(rng.uniform(300, 1500))), [None, 2, 3][i % 3], (-10.0, 10.0) if i % 2 else None,
                                   float(secs / np.float32(60.0)), id=f"t{i}"))
    tolu = ["ppm" if i % 4 == 1 else "Da" for i in range(20)]
    for name, nl in (("w.mgf", "\n"), ("w.mgf.gz", "\r\n")):
        write_mgf(str(tmp_path / name), spectra, tolu=tolu, newline=nl)
        b, kinds, zero = read_mgf_native(str(tmp_path / name))
        assert b.ids == [s.id for s in spectra]
        np.testing.assert_array_equal(bits(b.scan_start_time), bits([s.scan_start_time for s in spectra]))
        np.testing.assert_array_equal(bits(b.mz), bits(np.concatenate([s.mz for s in spectra])))
        np.testing.assert_array_equal(kinds, [R.TOL_PPM if (i % 2 and i % 4 == 1) else TOL_DA for i in range(20)])


def test_writer_quoting(tmp_path):
    from sage_amd import output
    assert output.csv_field("controllerType=0 scan=1") == "controllerType=0 scan=1"
    assert output.csv_field('File:"a.raw", NativeID:"scan=5"') == '"File:""a.raw"", NativeID:""scan=5"""'
    assert [output.csv_field(s) for s in ("a\tb", "a\rb", "a\nb", "")] == ['"a\tb"', '"a\rb"', '"a\nb"', ""]
    ids = ["scan=1", 'q"x', "t\tab", "plain id"]
    kw = dict(file_id=np.zeros(4, np.uint32), ion_injection_time=np.ones(4, np.float32), intensity=np.arange(8, dtype=np.float32))
    output.write_tmt_native(str(tmp_path / "native.tsv"), ["a", "b"], ["run 1.mgf"], spec_ids=ids, **kw)
    output.write_tmt(str(tmp_path / "twin.tsv"), ["a", "b"], output.tmt_rows(["run 1.mgf"], kw["file_id"], ids,
                                                                              kw["ion_injection_time"], kw["intensity"]))
    native = (tmp_path / "native.tsv").read_bytes()
    assert native == (tmp_path / "twin.tsv").read_bytes()
    lines = native.decode().split("\n")
    assert lines[1].startswith("run 1.mgf\tscan=1\t") and lines[2].startswith('run 1.mgf\t"q""x"\t')
    assert lines[3].startswith('run 1.mgf\t"t\tab"\t') and lines[4].startswith("run 1.mgf\tplain id\t")


@pytest.mark.parametrize("deisotope", [True, False], ids=["deisotope", "heap"])
def test_host_processing_of_peaks_in_file_order(deisotope):
    """MGF peaks come in file order: SpectrumProcessor::process uses them unsorted (deisotope's two pointers and
    bounded_min_heapify over the raw positions, spectrum.rs:179-227, 279-335).  The host restatement against the oracle's."""
    import oracle_lib
    import raw_spectra as G
    from sage_amd.api import SpectrumProcessor
    for k in range(300):
        rng = np.random.default_rng([k, int(deisotope), 77])
        n = G.peak_count(rng, huge=0.01)
        mz, it = G.raw_peaks(rng, n)
        order = rng.permutation(n) if k % 3 else np.arange(n)[::-1]  # shuffled, or descending
        mz, it = np.ascontiguousarray(mz[order]), np.ascontiguousarray(it[order])
        z = G.precursor_charge(rng)
        top_n = G.take_top_n(rng, n)
        min_mz = G.min_deisotope_mz(rng, [mz])
        p = SpectrumProcessor(top_n, deisotope, min_mz).process(RawSpectrum(mz, it, 500.0, z or None))
        om, oi, ot = oracle_lib.process_ms2(top_n, deisotope, min_mz, mz, it, z)
        ctx = f"case {k}: n={n} z={z} take_top_n={top_n}"
        np.testing.assert_array_equal(bits(p.masses), bits(om), err_msg=ctx)
        np.testing.assert_array_equal(bits(p.intensities), bits(oi), err_msg=ctx)
        assert bits(p.total_ion_current) == bits(ot), ctx
