"""mzML input for the search-and-score path (host side).

`read_mzml` follows the reference's reader, crates/sage-cloudpath/src/mzml.rs:109-403, for the fields the path uses:
  * binary arrays: base64, optional zlib (MS:1000574), 32- or 64-bit floats (MS:1000521 / MS:1000523), 64-bit values
    narrowed to f32 element-wise (:318-326);
  * numeric cvParam values are parsed straight to the target type: f32 for m/z, intensities, times (:139-147);
  * selected ion m/z (MS:1000744, ignored when 0), charge (MS:1000041), intensity (MS:1000042); isolation window target as
    the fallback precursor m/z (MS:1000827, :221-229); isolation_window = Da(-lower, +upper) when both offsets are present
    (:354-357); a precursor is kept only if its m/z != 0 (:353);
  * scan start time in minutes (seconds are divided by 60 in f32, :262-272); inverse reduced ion mobility (MS:1002815);
  * a spectrum whose total ion current cvParam is 0 is dropped (:205-213); an ms-level filter drops other levels;
  * ion injection time (MS:1000927 under <scan>, :273); the spectrumRef attribute of the kept precursor (:167-172);
  * signal-to-noise (`sn_level`, :371-381): at that MS level intensity[i] /= noise[i] (noise array MS:1002744, recognised
    only when the array is neither m/z nor intensity) over the shorter of the two arrays, in f32.  Only the spectrum's own
    noise array divides it; the reference would reuse an earlier spectrum's unused one.
  * per-peak ion mobility of MS1 spectra — an addition over the reference's mzML reader, which ignores the array: a
    binaryDataArray with one of MOBILITY_ARRAYS that is neither m/z, intensity nor noise becomes RawSpectrum.mobility (f32) of a
    spectrum whose ms level is 1; other levels drop it (spectrum.rs:344).  A length other than the m/z array's is an error.
`write_mzml` is ours (the reference has no writer): centroid MS2 spectra with 32-bit zlib arrays like the reference's
test fixture (tests/LQSRPAAPPAPGPGQLTLR.mzML:117-126), used to feed synthetic workloads through the CLI.
"""
import base64
import struct
import zlib
import xml.etree.ElementTree as ET
from xml.sax.saxutils import escape
from decimal import Decimal, InvalidOperation
from fractions import Fraction
from typing import List, Optional

import numpy as np

from .api import RawSpectrum

_F32 = np.float32

# ion mobility array, mean ion mobility array, mean inverse reduced ion mobility array, raw ion mobility array, raw inverse
# reduced ion mobility array (PSI-MS; matched by accession only)
MOBILITY_ARRAYS = ("MS:1002893", "MS:1002816", "MS:1003006", "MS:1003007", "MS:1003008")


def _local(tag: str) -> str:
    return tag.rsplit("}", 1)[-1]


def _f32(text: str) -> float:
    """Rust's str::parse::<f32>(): the decimal string rounded ONCE to the nearest f32 (ties to even).  float(text) rounds
    to f64 first; the neighbours of that result are compared exactly so a second rounding can never pick the wrong f32."""
    if not text:
        return 0.0
    try:
        exact = Fraction(Decimal(text.strip()))
    except (InvalidOperation, ValueError):
        return float(_F32(float(text)))  # inf / nan spellings
    c = _F32(float(text))
    if not np.isfinite(c):
        return float(c)
    best, best_err = c, abs(Fraction(float(c)) - exact)
    for cand in (np.nextafter(c, _F32(-np.inf)), np.nextafter(c, _F32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - exact)
        if err < best_err or (err == best_err and (int(np.array(cand).view(np.uint32)) & 1) == 0):
            best, best_err = cand, err
    return float(best)


def read_mzml(path: str, file_id: int = 0, ms_level: Optional[int] = 2, sn_level: Optional[int] = None) -> List[RawSpectrum]:
    """MzMLReader::with_file_id_and_level_filter(file_id, ms_level).set_signal_to_noise(sn_level).parse(..) for the MSn
    spectra of one file."""
    out: List[RawSpectrum] = []
    for _, el in ET.iterparse(path, events=("end",)):
        if _local(el.tag) != "spectrum":
            continue
        level, tic_zero = None, False
        for cv in el:
            if _local(cv.tag) != "cvParam":
                continue
            acc = cv.attrib.get("accession")
            if acc == "MS:1000511":
                level = int(cv.attrib["value"])
            elif acc == "MS:1000285":
                tic_zero = _f32(cv.attrib["value"]) == 0.0
        if tic_zero or (ms_level is not None and level != ms_level):
            el.clear()
            continue
        mz = np.zeros(0, _F32)
        inten = np.zeros(0, _F32)
        noise = mobility = None
        scan_start, iit, prec_ref = 0.0, 0.0, ""
        prec_mz, prec_charge, prec_ims = 0.0, None, None
        iso_lo = iso_hi = None
        have_precursor = False
        for sub in el.iter():
            t = _local(sub.tag)
            if t == "scan":
                for cv in sub:
                    if _local(cv.tag) != "cvParam":
                        continue
                    acc = cv.attrib.get("accession")
                    if acc == "MS:1000016":
                        v = _F32(_f32(cv.attrib["value"]))
                        unit = cv.attrib.get("unitAccession")
                        if unit == "UO:0000010":
                            v = _F32(v / _F32(60.0))
                        elif unit != "UO:0000031":
                            raise ValueError("malformed mzML: scan start time unit")
                        scan_start = float(v)
                    elif acc == "MS:1000927":
                        iit = _f32(cv.attrib["value"])
                    elif acc == "MS:1002815":
                        prec_ims = _f32(cv.attrib["value"])
            elif t == "precursor" and not have_precursor:  # the path reads precursors.first()
                p_mz, p_z, p_lo, p_hi = 0.0, None, None, None
                p_ref = sub.attrib.get("spectrumRef", "")
                for cv in sub.iter():
                    if _local(cv.tag) != "cvParam":
                        continue
                    acc, val = cv.attrib.get("accession"), cv.attrib.get("value", "")
                    if acc == "MS:1000827":
                        if p_mz == 0.0:
                            p_mz = _f32(val)
                    elif acc == "MS:1000828":
                        p_lo = _f32(val)
                    elif acc == "MS:1000829":
                        p_hi = _f32(val)
                    elif acc == "MS:1000041":
                        p_z = int(val)
                    elif acc == "MS:1000744":
                        v = _f32(val)
                        if v != 0.0:
                            p_mz = v
                    elif acc == "MS:1002815":
                        prec_ims = _f32(val)
                if p_mz != 0.0:
                    have_precursor = True
                    prec_mz, prec_charge = p_mz, p_z
                    iso_lo, iso_hi = p_lo, p_hi
                    prec_ref = p_ref
            elif t == "binaryDataArray":
                accs = [cv.attrib.get("accession") for cv in sub if _local(cv.tag) == "cvParam"]
                text = next((b.text for b in sub if _local(b.tag) == "binary"), None) or ""
                kind = ("mz" if "MS:1000514" in accs else "intensity" if "MS:1000515" in accs else
                        "noise" if "MS:1002744" in accs else "mobility" if any(a in MOBILITY_ARRAYS for a in accs) else None)
                if (not text or kind is None or (kind == "noise" and (sn_level is None or level != sn_level)) or
                        (kind == "mobility" and level != 1)):
                    continue
                raw = base64.b64decode(text)
                if "MS:1000574" in accs:
                    raw = zlib.decompress(raw)
                if "MS:1000521" in accs:
                    arr = np.frombuffer(raw[:len(raw) // 4 * 4], dtype="<f4").astype(_F32)
                else:
                    arr = np.frombuffer(raw[:len(raw) // 8 * 8], dtype="<f8").astype(_F32)
                if kind == "mz":
                    mz = arr
                elif kind == "intensity":
                    inten = arr
                elif kind == "mobility":
                    mobility = arr
                else:
                    noise = arr
        if noise is not None and len(noise):
            k = min(len(inten), len(noise))
            inten = inten.copy()
            with np.errstate(divide="ignore", invalid="ignore"):
                inten[:k] = inten[:k] / noise[:k]
        iso = (-iso_lo, iso_hi) if (iso_lo is not None and iso_hi is not None) else None
        if mobility is not None and len(mobility) != len(mz):
            raise ValueError(f"malformed mzML: ion mobility array of spectrum {el.attrib.get('id', '')} holds {len(mobility)} "
                             f"values for {len(mz)} m/z values")
        out.append(RawSpectrum(mz, inten, prec_mz, prec_charge, iso, scan_start, prec_ims, file_id, el.attrib.get("id", ""), iit,
                               prec_ref, mobility))
        el.clear()
    return out


def read_mzml_native(path: str, file_id: int = 0, ms_level: Optional[int] = 2, check_searchable: bool = False,
                     sn_level: Optional[int] = None):
    """The same reader in C++ (csrc/mzml_reader.cpp, sage_hip_mzml_read): one call per file, arrays straight into a RawBatch
    for Scorer.process_upload — no Python object per spectrum.  gzip-compressed files are inflated on the way in.
    check_searchable: refuse what the reference refuses to search (profile-mode MS2 spectra, MS2 spectra without precursor).
    sn_level: divide the intensities of that MS level by their noise array (sage_hip_mzml_read_sn)."""
    import ctypes as C

    from . import _lib as L
    from .api import RawBatch
    lib = L.load()
    h = C.c_void_p()
    level = -1 if ms_level is None else int(ms_level)
    if sn_level is None:
        L.check(lib.sage_hip_mzml_read(path.encode(), file_id, level, C.byref(h)))
    else:
        L.check(lib.sage_hip_mzml_read_sn(path.encode(), file_id, level, int(sn_level), C.byref(h)))
    try:
        if check_searchable:
            L.check(lib.sage_hip_mzml_check_searchable(h))
        v = L.SageRawBatch()
        L.check(lib.sage_hip_mzml_view(h, C.byref(v)))
        n = int(v.n_spectra)

        def arr(ptr, count, dtype):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True)

        peak_off = arr(v.peak_off, n + 1, np.uint64)
        npk = int(peak_off[-1])
        mob_ptr = lib.sage_hip_mzml_mobility(h)
        mobility = has_mobility = None
        if mob_ptr:
            mobility = arr(mob_ptr, npk, np.float32)
            has_mobility = np.zeros(max(n, 1), np.uint8)
            L.check(lib.sage_hip_mzml_has_mobility(h, L.as_ptr(has_mobility, C.c_uint8)))
            has_mobility = has_mobility[:n]
        ids = [lib.sage_hip_mzml_spectrum_id(h, i).decode() for i in range(n)]
        return RawBatch.from_arrays(ids, peak_off, arr(v.mz, npk, np.float32), arr(v.intensities, npk, np.float32),
                                    arr(v.precursor_mz, n, np.float32), arr(v.precursor_charge, n, np.uint8),
                                    arr(v.isolation_lo, n, np.float32), arr(v.isolation_hi, n, np.float32),
                                    arr(v.scan_start_time, n, np.float32), arr(v.inverse_ion_mobility, n, np.float32),
                                    arr(v.file_id, n, np.uint32),
                                    np.array([lib.sage_hip_mzml_ion_injection_time(h, i) for i in range(n)], dtype=np.float32),
                                    [lib.sage_hip_mzml_precursor_ref(h, i).decode() for i in range(n)],
                                    mobility=mobility, has_mobility=has_mobility)
    finally:
        lib.sage_hip_mzml_free(h)


def _b64(arr: np.ndarray, bits: int = 32, compress: bool = True) -> str:
    raw = np.ascontiguousarray(arr, dtype="<f4" if bits == 32 else "<f8").tobytes()
    return base64.b64encode(zlib.compress(raw) if compress else raw).decode()


def write_mzml(path: str, spectra: List[RawSpectrum], ms_levels: Optional[List[int]] = None, noise=None,
               extra_precursors=None, mobility=None, mobility_encoding=(MOBILITY_ARRAYS[0], 32, True)) -> None:
    """Centroid MS2 spectra, 32-bit zlib arrays, selected ion m/z / charge, isolation offsets, scan start time (minutes).
    ms_levels: per spectrum (default 2); an `ms level` 1 spectrum is written without a precursor list.  A non-zero
    ion_injection_time, a non-empty precursor_ref (spectrumRef) and an inverse_ion_mobility (MS:1002815 under <scan>) are written
    when set.  noise: per spectrum, a noise array
    (MS:1002744) or None; extra_precursors: per spectrum, further precursor m/z (SPS-MS3) after the first, or None.
    mobility: per spectrum, a per-peak ion-mobility array or None (written at any ms level: the reader keeps it at level 1),
    after the noise array; mobility_encoding: its (accession, 32 or 64 bits, zlib or not)."""
    with open(path, "w") as f:
        f.write('<?xml version="1.0" encoding="utf-8"?>\n<mzML xmlns="http://psi.hupo.org/ms/mzml" version="1.1.0">\n')
        f.write(f'<run id="synthetic"><spectrumList count="{len(spectra)}">\n')
        for i, s in enumerate(spectra):
            sid = s.id or f"scan={i + 1}"
            f.write(f'<spectrum index="{i}" id="{sid}" defaultArrayLength="{len(s.mz)}">\n')
            level = 2 if ms_levels is None else int(ms_levels[i])
            f.write(f'<cvParam cvRef="MS" accession="MS:1000511" name="ms level" value="{level}"/>\n')
            f.write('<cvParam cvRef="MS" accession="MS:1000127" name="centroid spectrum"/>\n')
            iit = getattr(s, "ion_injection_time", 0.0)
            iit_cv = (f'<cvParam cvRef="MS" accession="MS:1000927" name="ion injection time" '
                      f'value="{np.format_float_positional(np.float32(iit), unique=True)}"/>' if iit else "")
            ims = getattr(s, "inverse_ion_mobility", None)
            if ims is not None:
                iit_cv += (f'<cvParam cvRef="MS" accession="MS:1002815" name="inverse reduced ion mobility" '
                           f'value="{np.format_float_positional(np.float32(ims), unique=True)}"/>')
            f.write(f'<scanList count="1"><scan><cvParam cvRef="MS" accession="MS:1000016" name="scan start time" '
                    f'value="{np.format_float_positional(np.float32(s.scan_start_time), unique=True)}" unitCvRef="UO" '
                    f'unitAccession="UO:0000031" unitName="minute"/>{iit_cv}</scan></scanList>\n')
            nz = None if noise is None else noise[i]
            mob = None if mobility is None or mobility[i] is None else (mobility[i],) + tuple(mobility_encoding)
            if level == 1:
                _write_arrays(f, s, nz, mob)
                continue
            ref = getattr(s, "precursor_ref", "")
            extra = [] if extra_precursors is None or extra_precursors[i] is None else list(extra_precursors[i])
            ref_attr = f' spectrumRef="{escape(ref, {chr(34): "&quot;"})}"' if ref else ""
            f.write(f'<precursorList count="{1 + len(extra)}"><precursor{ref_attr}>')
            if s.isolation_window is not None:
                lo, hi = s.isolation_window
                f.write('<isolationWindow>'
                        f'<cvParam cvRef="MS" accession="MS:1000827" name="isolation window target m/z" value="{np.format_float_positional(np.float32(s.precursor_mz), unique=True)}"/>'
                        f'<cvParam cvRef="MS" accession="MS:1000828" name="isolation window lower offset" value="{np.format_float_positional(np.float32(-lo), unique=True)}"/>'
                        f'<cvParam cvRef="MS" accession="MS:1000829" name="isolation window upper offset" value="{np.format_float_positional(np.float32(hi), unique=True)}"/>'
                        '</isolationWindow>')
            f.write('<selectedIonList count="1"><selectedIon>'
                    f'<cvParam cvRef="MS" accession="MS:1000744" name="selected ion m/z" value="{np.format_float_positional(np.float32(s.precursor_mz), unique=True)}"/>')
            if s.precursor_charge:
                f.write(f'<cvParam cvRef="MS" accession="MS:1000041" name="charge state" value="{int(s.precursor_charge)}"/>')
            f.write('</selectedIon></selectedIonList></precursor>')
            for x in extra:
                f.write(f'<precursor{ref_attr}><selectedIonList count="1"><selectedIon><cvParam cvRef="MS" accession="MS:1000744" '
                        f'name="selected ion m/z" value="{np.format_float_positional(np.float32(x), unique=True)}"/>'
                        '</selectedIon></selectedIonList></precursor>')
            f.write('</precursorList>\n')
            _write_arrays(f, s, nz, mob)
        f.write('</spectrumList></run></mzML>\n')


def _write_arrays(f, s, noise=None, mobility=None) -> None:
    arrays = [("MS:1000514", "m/z array", s.mz), ("MS:1000515", "intensity array", s.intensity)]
    if noise is not None:
        arrays.append(("MS:1002744", "sampled noise intensity array", noise))
    f.write(f'<binaryDataArrayList count="{len(arrays) + (mobility is not None)}">')
    for acc, name, arr in arrays:
        f.write('<binaryDataArray><cvParam cvRef="MS" accession="MS:1000521" name="32-bit float"/>'
                '<cvParam cvRef="MS" accession="MS:1000574" name="zlib compression"/>'
                f'<cvParam cvRef="MS" accession="{acc}" name="{name}"/><binary>{_b64(arr)}</binary></binaryDataArray>')
    if mobility is not None:
        arr, acc, bits, compress = mobility
        width = ('<cvParam cvRef="MS" accession="MS:1000521" name="32-bit float"/>' if bits == 32 else
                 '<cvParam cvRef="MS" accession="MS:1000523" name="64-bit float"/>')
        comp = ('<cvParam cvRef="MS" accession="MS:1000574" name="zlib compression"/>' if compress else
                '<cvParam cvRef="MS" accession="MS:1000576" name="no compression"/>')
        f.write(f'<binaryDataArray>{width}{comp}<cvParam cvRef="MS" accession="{acc}" name="ion mobility array"/>'
                f'<binary>{_b64(arr, bits, compress)}</binary></binaryDataArray>')
    f.write('</binaryDataArrayList>\n</spectrum>\n')
