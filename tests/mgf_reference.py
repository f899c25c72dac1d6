"""Sequential restatement of the reference's MGF reader, from crates/sage-cloudpath/src/mgf.rs and util.rs alone.

read_mgf(text) follows MgfReader::parse (mgf.rs:325-369) one line at a time: the file-level section up to the first line that
starts with BEGIN IONS (DefaultParser, :131-182), then the query parsers in their order mz, end, pepmass, title, charge, tol,
tolu, rt (QueryParser, :184-322), the first Ok(true) winning.  QueryData starts WITHOUT the defaults (default_with_params,
:55-60); init() at END IONS copies them in (:61-70).  Numbers go through rust_f32 (core's dec2flt: grammar + correct rounding),
restated here with exact rational arithmetic.  Returns dicts with the fields of RawSpectrum + precursors[0] the path reads.
"""
import re
from fractions import Fraction

import numpy as np

TOL_PPM, TOL_DA = 0, 2

_FLOAT = re.compile(r"[+-]?(\d+|\d+\.\d*|\d*\.\d+)([eE][+-]?\d+)?\Z")
_SPECIAL = {"inf": float("inf"), "infinity": float("inf"), "nan": float("nan")}
_MAX = Fraction(2) ** 128 - Fraction(2) ** 103  # f32::MAX
_HALF_ULP_MAX = Fraction(2) ** 103              # half the spacing at f32::MAX (2^104 / 2)


def _round_f32(q: Fraction) -> np.float32:
    """the f32 nearest to q >= 0, ties to even (IEEE round-to-nearest-even), inf beyond f32::MAX + half an ulp"""
    if q == 0:
        return np.float32(0.0)
    if q >= _MAX + _HALF_ULP_MAX:
        return np.float32(np.inf)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)  # subnormals share the exponent of the smallest normal
    ulp = Fraction(2) ** (e - 23)
    k = q / ulp
    n = k.numerator // k.denominator
    rem = k - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    v = n * ulp
    if v > _MAX:
        return np.float32(np.inf)
    return np.float32(float(v))  # (exact: v has at most 24 significant bits)


def rust_f32(token: str):
    """str::parse::<f32>(): the np.float32 value, or None when rejected"""
    body = token[1:] if token[:1] in "+-" else token
    neg = token[:1] == "-"
    if body.lower() in _SPECIAL:
        v = np.float32(_SPECIAL[body.lower()])
        return np.float32(-v) if neg else v
    if not _FLOAT.match(token) or not token.isascii():
        return None
    mant, _, exp = body.lower().partition("e")
    ip, _, fp = mant.partition(".")
    digits = (ip + fp).lstrip("0")
    x = int(exp) - len(fp) if exp else -len(fp)
    if not digits:
        v = np.float32(0.0)
    elif x + len(digits) > 50:  # above 1e50: beyond f32::MAX
        v = np.float32(np.inf)
    elif x + len(digits) < -60:  # below 1e-60: under half the smallest subnormal (1.4e-45)
        v = np.float32(0.0)
    else:
        v = _round_f32(Fraction(int(digits)) * Fraction(10) ** x)
    return np.float32(-v) if neg else v


# char::is_whitespace (Unicode White_Space), for str::trim
_WS = "".join(map(chr, [*range(0x09, 0x0E), 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]))
_ASCII_WS = " \t\n\x0c\r"  # u8::is_ascii_whitespace (split_ascii_whitespace)


def rust_lines(text: str):
    """str::lines(): split at \\n, one trailing \\r dropped, no final empty line"""
    parts = text.split("\n")
    if parts and parts[-1] == "":
        parts.pop()
    return [p[:-1] if p.endswith("\r") else p for p in parts]


def split_ascii_ws(s: str):
    return [t for t in re.split("[" + re.escape(_ASCII_WS) + "]+", s) if t]


def charges_of(s: str):
    """regex (\\d)\\+? over the value: every Unicode digit matches; to_digit(10) keeps only the ASCII ones"""
    return [int(c) for c in s if "0" <= c <= "9"]


class _Query:
    def __init__(self, defaults):
        self.d = defaults
        self.id, self.prec, self.rt = "", [], None
        self.tol = self.unit = self.charges = None  # default_with_params: the defaults are NOT copied in
        self.mz, self.inten = [], []
        self.spectra, self.dropped = [], []

    def init(self):
        self.id, self.prec, self.rt = "", [], None
        self.tol, self.unit, self.charges = self.d["tol"], self.d["unit"], (None if self.d["charges"] is None else list(self.d["charges"]))
        self.mz, self.inten = [], []

    def end(self, file_id):
        precursors = []
        for p in self.prec:  # get_precursors_with_charge (:86-104)
            if self.charges is not None:
                precursors += [(p, c) for c in self.charges]
            else:
                precursors.append((p, None))
        window = None
        if self.tol is not None and self.unit in ("Da", "ppm"):
            t = np.float32(abs(self.tol))
            window = (TOL_DA if self.unit == "Da" else TOL_PPM, np.float32(-t), t)
        if not self.id or not precursors or not self.mz or len(self.mz) != len(self.inten):
            self.dropped.append(self.id)
        else:
            mz, charge = precursors[0]
            self.spectra.append(dict(
                id=self.id, precursor_mz=np.float32(mz), charge=charge, isolation=window, file_id=file_id,
                scan_start_time=np.float32(0.0) if self.rt is None else self.rt,
                mz=np.array(self.mz, np.float32), intensity=np.array(self.inten, np.float32)))
        self.init()

    def line(self, line, file_id):
        if line[:1].isdigit():  # parse_mz (a non-ASCII numeric first char: its token fails to parse, nothing is added)
            toks = split_ascii_ws(line)
            mz = rust_f32(toks[0])
            if mz is None:
                return
            self.mz.append(mz)
            if len(toks) > 1:
                x = rust_f32(toks[1])
                if x is not None:
                    self.inten.append(x)
            else:
                self.inten.append(np.float32(1.0))
            return
        if line.startswith("END IONS"):
            return self.end(file_id)
        if line.startswith("PEPMASS="):
            toks = split_ascii_ws(line[8:])
            mz = np.float32(0.0)
            if toks:
                mz = rust_f32(toks[0])
                if mz is None:
                    return
            self.prec.append(mz)
            return
        if line.startswith("TITLE="):
            self.id = line[6:]
            return
        if line.startswith("CHARGE="):
            self.charges = charges_of(line[7:])
            return
        if line.startswith("TOL="):
            v = rust_f32(line[4:])
            if v is not None:
                self.tol = v
            return
        if line.startswith("TOLU="):
            self.unit = line[5:]
            return
        if line.startswith("RTINSECONDS="):
            v = rust_f32(line[12:])
            if v is not None:
                self.rt = np.float32(v / np.float32(60.0))


def read_mgf(text: str, file_id: int = 0):
    """MgfReader::with_file_id(file_id).parse(text) -> (spectra, ids of dropped spectra).  ValueError where the reference
    panics (no BEGIN IONS)."""
    lines = rust_lines(text)
    d = dict(tol=None, unit=None, charges=None)
    k = 0
    while True:
        if k >= len(lines):
            raise ValueError("no BEGIN IONS")  # lines.next().unwrap()
        line = lines[k].strip(_WS)
        k += 1
        if line.startswith("BEGIN IONS"):
            break
        if line.startswith("TOL="):
            v = rust_f32(line[4:])
            if v is not None:
                d["tol"] = v
        elif line.startswith("TOLU="):
            d["unit"] = line[5:]
        elif line.startswith("CHARGE="):
            d["charges"] = charges_of(line[7:])
    q = _Query(d)
    for line in lines[k:]:
        if not line:
            continue
        q.line(line.strip(_WS), file_id)
    return q.spectra, q.dropped


def file_format(path: str) -> str:
    """FileFormat::from (util.rs:31-43) for the formats this project reads"""
    p = path.lower()
    if p.endswith(".mgf.gz") or p.endswith(".mgf"):
        return "mgf"
    return "mzml"
