"""MGF input (host side): sage-cloudpath's `read_mgf` (mgf.rs, util.rs:107-118) and the extension dispatch of `read_spectra`
(util.rs:31-43, :60-71).

`read_mgf_native` is the C++ reader (csrc/mgf_reader.cpp, sage_hip_mgf_read).  Besides the RawBatch it returns what an mzML
run never carries: the kind of each isolation window (`TOLU=ppm` gives Tolerance::Ppm, SAGE_TOL_PPM) and which spectra have
precursors[0].charge == Some(0), which RawBatch.precursor_charge == 0 ("no charge") cannot express.
`write_mgf` writes synthetic spectra for tests and benchmarks.
"""
import ctypes as C
import os
from typing import List, Optional, Tuple

import numpy as np

from .api import RawSpectrum

TOL_PPM, TOL_PCT, TOL_DA = 0, 1, 2  # SAGE_TOL_* (mass.rs:10-16)


def is_mgf(path: str) -> bool:
    """FileFormat::from (util.rs:31-43): the lower-cased path ends in .mgf or .mgf.gz"""
    p = str(path).lower()
    return p.endswith(".mgf.gz") or p.endswith(".mgf")


def read_mgf_native(path: str, file_id: int = 0) -> Tuple["RawBatch", np.ndarray, np.ndarray]:  # noqa: F821
    """Every spectrum of an MGF file: (RawBatch, isolation-window kinds uint8[n] (TOL_DA / TOL_PPM; NaN bounds == None),
    charge_zero uint8[n] (1 where the annotated charge of precursors[0] is 0)).  gzip-compressed files are inflated on the
    way in.  Raises SageHipError for a missing file, a file without BEGIN IONS or text that is not UTF-8."""
    from . import _lib as L
    from .api import RawBatch
    lib = L.load()
    h = C.c_void_p()
    L.check(lib.sage_hip_mgf_read(os.fsencode(path), file_id, C.byref(h)))
    try:
        v = L.SageRawBatch()
        L.check(lib.sage_hip_mzml_view(h, C.byref(v)))
        n = int(v.n_spectra)

        def arr(ptr, count, dtype):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True)

        peak_off = arr(v.peak_off, n + 1, np.uint64)
        npk = int(peak_off[-1])
        ids = [lib.sage_hip_mzml_spectrum_id(h, i).decode() for i in range(n)]
        kinds = np.zeros(n, np.uint8)
        zero = np.zeros(n, np.uint8)
        L.check(lib.sage_hip_mzml_isolation_kinds(h, L.as_ptr(kinds, C.c_uint8)))
        L.check(lib.sage_hip_mzml_charge_zero(h, L.as_ptr(zero, C.c_uint8)))
        batch = RawBatch.from_arrays(ids, peak_off, arr(v.mz, npk, np.float32), arr(v.intensities, npk, np.float32),
                                     arr(v.precursor_mz, n, np.float32), arr(v.precursor_charge, n, np.uint8),
                                     arr(v.isolation_lo, n, np.float32), arr(v.isolation_hi, n, np.float32),
                                     arr(v.scan_start_time, n, np.float32), arr(v.inverse_ion_mobility, n, np.float32),
                                     arr(v.file_id, n, np.uint32))
        return batch, kinds, zero
    finally:
        lib.sage_hip_mzml_free(h)


def parse_f32(token: str) -> Optional[float]:
    """str::parse::<f32>() as the native MGF reader applies it: the f32 value, or None when the token is rejected"""
    from . import _lib as L
    raw = token.encode()
    out = C.c_float()
    if L.load().sage_hip_parse_f32(raw, len(raw), C.byref(out)) != 0:
        return None
    return out.value


def read_spectra(path: str, file_id: int = 0, ms_level: Optional[int] = 2, check_searchable: bool = False,
                 sn_level: Optional[int] = None):
    """sage-cloudpath read_spectra (util.rs:60-71): MGF by extension, everything else to the mzML reader as before.
    Returns (RawBatch, isolation-window kinds, charge_zero).  MGF holds MS2 spectra only, so any other ms_level reads none,
    and read_mgf takes no signal-to-noise level: sn_level is ignored for MGF.  mzML runs carry Da windows and no charge 0."""
    if is_mgf(path):
        batch, kinds, zero = read_mgf_native(path, file_id=file_id)
        if ms_level is not None and int(ms_level) != 2:
            batch = batch.subset(np.zeros(0, np.int64))
            kinds, zero = kinds[:0], zero[:0]
        return batch, kinds, zero
    from .mzml import read_mzml_native
    batch = read_mzml_native(path, file_id=file_id, ms_level=ms_level, check_searchable=check_searchable, sn_level=sn_level)
    return batch, np.full(batch.n, TOL_DA, np.uint8), np.zeros(batch.n, np.uint8)


def _f32_text(x) -> str:
    return np.format_float_positional(np.float32(x), unique=True)


def write_mgf(path: str, spectra: List[RawSpectrum], tolu: Optional[List[Optional[str]]] = None,
              header: str = "", newline: str = "\n") -> None:
    """One BEGIN IONS block per spectrum: TITLE (s.id), RTINSECONDS (f32(scan_start_time * 60)), PEPMASS, CHARGE (when set),
    TOL / TOLU for an isolation window (|hi|; `tolu[i]`, default "Da") and the peaks as shortest round-trip f32 text.  Spectra
    whose scan_start_time is f32(seconds) / 60 read back bit for bit.  `header` is written before the first BEGIN IONS (file
    defaults, which the reference applies from the second spectrum on); a path ending in .gz is gzip-compressed."""
    out = [header]
    for i, s in enumerate(spectra):
        b = ["BEGIN IONS", f"TITLE={s.id}", f"RTINSECONDS={_f32_text(np.float32(s.scan_start_time) * np.float32(60.0))}",
             f"PEPMASS={_f32_text(s.precursor_mz)}"]
        if s.precursor_charge is not None:
            b.append(f"CHARGE={int(s.precursor_charge)}+")
        if s.isolation_window is not None:
            b.append(f"TOL={_f32_text(abs(s.isolation_window[1]))}")
            b.append(f"TOLU={(tolu[i] if tolu is not None and tolu[i] else 'Da')}")
        b += [f"{_f32_text(m)} {_f32_text(x)}" for m, x in zip(s.mz, s.intensity)]
        b.append("END IONS")
        out.append(newline.join(b) + newline)
    data = "".join(out).encode()
    if str(path).endswith(".gz"):
        import gzip
        data = gzip.compress(data)
    with open(path, "wb") as f:
        f.write(data)
