"""A plain numpy restatement of the fragment index that sage_hip_db_create derives in HBM, written from the
reference's source lines and from the layouts' definitions — not from index_build.hip or capi_db.hip:

* the ion table: IonSeries::new / next (ion_series.rs:36-85) of every peptide and configured kind, an f32 running sum in sequence
  order (np.cumsum over a 1-D f32 array accumulates sequentially), residue masses of mass.rs:64-76;
* the stored entries: the filter of Parameters::build_from_peptides (database.rs:281-292);
* a tile-major copy for tiles of 2^s peptides: the stored entries ordered by (peptide >> s, f32::total_cmp of m/z, peptide), then
  two padding entries;
* its row-major position table, the succinct form of that table (occupancy bits, ranks, run starts) and the decoding of the
  succinct form back into rows;
* the peptide-mass table, pep_info, the |ion| range.

tests/test_index_reference_cpu.py holds this module to the oracle and to the host build; tests/test_gpu_index_tables.py holds the
device's tables to this module."""
import ctypes as C

import numpy as np

from sage_amd import _lib as L

F32 = np.float32
PAD = np.array([(0xFFFFFFFF, 0.0)], dtype=L.THEORETICAL_DTYPE)

# mass.rs:64-68: A..Z (B, J, X, Z: 0); any other byte: 0 (mass.rs:70-76)
MONOISOTOPIC_MASSES = np.array([
    71.03711, 0.0, 103.00919, 115.02694, 129.04259, 147.0684, 57.02146, 137.05891, 113.08406, 0.0,
    128.09496, 113.08406, 131.0405, 114.04293, 237.14774, 97.05276, 128.05858, 156.1011, 87.03203,
    101.04768, 150.95363, 99.06841, 186.07932, 0.0, 163.06332, 0.0], dtype=F32)
RESIDUE_MASS = np.zeros(256, dtype=F32)
RESIDUE_MASS[ord("A"):ord("Z") + 1] = MONOISOTOPIC_MASSES

# ion_series.rs:37-42
_C, _O, _H, _PRO, _N = F32(12.0), F32(15.994914), F32(1.007825), F32(1.0072764), F32(14.003074)
_NH3 = F32(F32(_N + F32(_H * F32(2.0))) + _PRO)
_CO = F32(_C + _O)
_X_SHIFT = F32(F32(F32(F32(_CO - _NH3) + _N)) + _H)  # C + O - NH3 + N + H, left to right
KIND_A, KIND_B, KIND_C, KIND_X, KIND_Y, KIND_Z = range(6)


def total_order_key(x):
    """f32::total_cmp as an integer key (i64): a < b in the total order iff key(a) < key(b).  The bit pattern as i32, with the
    31 low bits of negative values flipped."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def popcount32(x):
    x = np.ascontiguousarray(x, dtype=np.uint32)
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x).astype(np.uint32)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (4,)), axis=-1).sum(axis=-1, dtype=np.uint32)


def _first_mass(kind, nterm, mono):
    nt = F32(0.0) if np.isnan(nterm) else F32(nterm)  # Option::unwrap_or_default
    if kind == KIND_A:
        return F32(nt - _CO)
    if kind == KIND_B:
        return nt
    if kind == KIND_C:
        return F32(nt + _NH3)
    if kind == KIND_X:
        return F32(F32(mono - nt) + _X_SHIFT)
    if kind == KIND_Y:
        return F32(mono - nt)
    assert kind == KIND_Z
    return F32(F32(mono - nt) - _NH3)


class ArrayDb:
    """A SageDbView over numpy arrays (which it keeps alive): what DeviceDatabase needs of a host database — `_view` and
    `has_fragments` — for a hand-built peptide list, without the digest.  `fragments` (L.THEORETICAL_DTYPE, as IndexedDatabase.fragments
    holds them: every stored entry once) makes it a view WITH fragments: the host branch of sage_hip_db_create."""

    def __init__(self, sequences, mods=None, nterm=None, pep_mono=None, ion_kinds=(KIND_B, KIND_Y), min_ion_index=2, decoy=None,
                 missed_cleavages=None, fragments=None):
        n = len(sequences)
        lens = np.array([len(s) for s in sequences], dtype=np.uint64)
        self.seq_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(lens, out=self.seq_off[1:])
        self.seq = np.frombuffer(b"".join(bytes(s) for s in sequences), dtype=np.uint8).copy()
        self.mods = np.zeros(len(self.seq), F32) if mods is None else np.concatenate([np.asarray(m, F32) for m in mods] + [np.zeros(0, F32)])
        assert len(self.mods) == len(self.seq)
        self.nterm = np.full(n, np.nan, F32) if nterm is None else np.asarray(nterm, F32).copy()
        self.cterm = np.full(n, np.nan, F32)
        self.pep_mono = np.asarray(pep_mono, F32).copy()
        self.decoy = np.zeros(n, np.uint8) if decoy is None else np.asarray(decoy, np.uint8).copy()
        self.missed_cleavages = np.zeros(n, np.uint8) if missed_cleavages is None else np.asarray(missed_cleavages, np.uint8).copy()
        self.ion_kinds = np.asarray(ion_kinds, np.uint8).copy()
        self.min_ion_index = int(min_ion_index)
        self.n_peptides = n
        assert len(self.nterm) == len(self.pep_mono) == len(self.decoy) == len(self.missed_cleavages) == n
        self.fragments = None if fragments is None else np.ascontiguousarray(fragments, dtype=L.THEORETICAL_DTYPE)
        self.has_fragments = fragments is not None
        # (a pointer into an empty array is never read; give ctypes a real one all the same)
        self._keep = {k: (a if len(a) else np.zeros(1, a.dtype)) for k, a in self.__dict__.items() if isinstance(a, np.ndarray)}
        v = self._view = L.SageDbView()
        k = self._keep
        if self.has_fragments:
            v.fragments = k["fragments"].ctypes.data_as(C.POINTER(L.SageTheoretical))
            v.n_fragments = len(self.fragments)
        v.pep_mono = L.as_ptr(k["pep_mono"], C.c_float)
        v.seq_off = L.as_ptr(k["seq_off"], C.c_uint64)
        v.seq = L.as_ptr(k["seq"], C.c_uint8)
        v.mods = L.as_ptr(k["mods"], C.c_float)
        v.nterm = L.as_ptr(k["nterm"], C.c_float)
        v.cterm = L.as_ptr(k["cterm"], C.c_float)
        v.decoy = L.as_ptr(k["decoy"], C.c_uint8)
        v.missed_cleavages = L.as_ptr(k["missed_cleavages"], C.c_uint8)
        v.n_peptides = n
        v.ion_kinds = L.as_ptr(k["ion_kinds"], C.c_uint8)
        v.n_ion_kinds = len(self.ion_kinds)
        v.min_ion_index = self.min_ion_index

    def with_fragments(self, fragments):
        """The same peptides as a view with fragments."""
        off = self.seq_off.astype(np.int64)
        return ArrayDb([self.seq[off[i]:off[i + 1]].tobytes() for i in range(self.n_peptides)],
                       [self.mods[off[i]:off[i + 1]] for i in range(self.n_peptides)], self.nterm, self.pep_mono, self.ion_kinds,
                       self.min_ion_index, self.decoy, self.missed_cleavages, fragments)


class IndexReference:
    """The tables of one database.  `db`: anything with the arrays of a SageDbView as attributes (an api.IndexedDatabase, an
    ArrayDb); min_ion_index is taken from its view unless given."""

    def __init__(self, db, min_ion_index=None):
        self.np = n = len(db.pep_mono)
        self.min_ion_index = mi = int(db._view.min_ion_index if min_ion_index is None else min_ion_index)
        self.kinds = kinds = [int(k) for k in db.ion_kinds]
        self.pep_mono = np.asarray(db.pep_mono, F32)
        off = np.asarray(db.seq_off).astype(np.int64)
        lens = off[1:] - off[:-1] if n else np.zeros(0, np.int64)
        lm1 = np.maximum(lens - 1, 0)
        nk = len(kinds)
        self.max_len = int(lens.max()) if n else 0
        self.max_ions = int((lm1 * nk).max()) if n else 0
        self.pep_info = (lens | (np.asarray(db.decoy).astype(np.int64) != 0).astype(np.int64) << 16 |
                         np.asarray(db.missed_cleavages).astype(np.int64) << 24).astype(np.uint32)
        self.ion_off = np.zeros(n + 1, np.uint64)
        np.cumsum(lm1 * nk, out=self.ion_off[1:])
        self.pm_off = np.zeros(n + 1, np.uint64)
        np.cumsum(np.maximum(lm1 - mi, 0) * nk, out=self.pm_off[1:])
        # monoisotopic(r) + m, f32 (ion_series.rs:75-78)
        step = (RESIDUE_MASS[np.asarray(db.seq, np.uint8)] + np.asarray(db.mods, F32)).astype(F32) if len(db.seq) else np.zeros(0, F32)
        ions, keep, pep = [], [], []
        for p in range(n):
            m = int(lm1[p])
            if not m:
                continue
            st = step[off[p]:off[p] + m]
            idx = np.arange(m)
            for kind in kinds:
                forward = kind in (KIND_A, KIND_B, KIND_C)
                run = np.empty(m + 1, F32)
                run[0] = _first_mass(kind, db.nterm[p], self.pep_mono[p])
                run[1:] = st if forward else -st
                ions.append(np.cumsum(run, dtype=F32)[1:])
                keep.append((idx + 1) > mi if forward else (m - idx) > mi)  # database.rs:285-289
            pep.append(np.full(m * nk, p, np.uint32))
        self.ions = np.concatenate(ions) if ions else np.zeros(0, F32)
        keep = np.concatenate(keep) if keep else np.zeros(0, bool)
        pep = np.concatenate(pep) if pep else np.zeros(0, np.uint32)
        assert len(self.ions) == int(self.ion_off[-1])
        # the stored entries, in generated order: peptide, kind, ion index
        self.entries = np.zeros(int(keep.sum()), dtype=L.THEORETICAL_DTYPE)
        self.entries["peptide_index"] = pep[keep]
        self.entries["fragment_mz"] = self.ions[keep]
        self.nf = len(self.entries)
        assert self.nf == int(self.pm_off[-1])
        a = self.ions.view(np.uint32) & np.uint32(0x7FFFFFFF)
        self.ion_lo_bits, self.ion_hi_bits = (int(a.min()), int(a.max())) if len(a) else (0xFFFFFFFF, 0)
        self._copies = {}  # tile_copy's results by shift (a module's tests share one IndexReference per database)

    def restricted_ion_table(self):
        """(peptide, m/z) of the ion table's entries that the keep rule stores — by peptide, kind and ion index from the offsets
        alone (a second way to the stored entries: test_index_reference_cpu.py)."""
        out_p, out_m = [], []
        nk = len(self.kinds)
        for p in range(self.np):
            m = (int(self.ion_off[p + 1]) - int(self.ion_off[p])) // nk if nk else 0
            for k, kind in enumerate(self.kinds):
                lo = int(self.ion_off[p]) + k * m
                sl = slice(lo + self.min_ion_index, lo + m) if kind <= KIND_C else slice(lo, lo + max(m - self.min_ion_index, 0))
                out_m.append(self.ions[sl])
                out_p.append(np.full(len(out_m[-1]), p, np.uint32))
        return (np.concatenate(out_p), np.concatenate(out_m)) if out_p else (np.zeros(0, np.uint32), np.zeros(0, F32))

    def sorted_entries(self):
        """The stored entries by (total-order key of m/z, peptide)."""
        e = self.entries
        return e[np.lexsort((e["peptide_index"], total_order_key(e["fragment_mz"])))]

    def peptide_major_sorted(self):
        """The stored entries by (peptide, total-order key of m/z) and the two padding entries: tiles of one peptide."""
        return self.tile_copy(0)

    def n_tiles(self, shift):
        return max(1, (self.np + (1 << shift) - 1) >> shift)

    def tile_offsets(self, shift):
        t = np.arange(self.n_tiles(shift) + 1, dtype=np.int64)
        return self.pm_off[np.minimum(t << shift, self.np)].astype(np.int64)

    def tile_copy(self, shift):
        """The stored entries in np.lexsort order of (peptide >> shift, total-order key of m/z, peptide), then two padding entries.
        (The first two keys travel in one u64 word, tile << 32 | key + 2^31: one sort fewer for the same order.)"""
        if shift not in self._copies:
            e = self.entries
            tile_key = ((e["peptide_index"] >> np.uint32(shift)).astype(np.uint64) << np.uint64(32)) | \
                (total_order_key(e["fragment_mz"]) + (1 << 31)).astype(np.uint64)
            self._copies[shift] = np.concatenate([e[np.lexsort((e["peptide_index"], tile_key))], PAD, PAD])
        return self._copies[shift]

    def stride(self, scale):
        mz = self.entries["fragment_mz"]
        ok = np.isfinite(mz) & (mz > 0)
        top = float(mz[ok].max()) if ok.any() else 0.0
        return int(min(np.ceil(top * float(scale)) + 3.0, 64e6))

    def position_table(self, shift, scale, tiles=None):
        """[n_tiles, stride] u32 (tiles: the rows of these tiles only)"""
        copy = self.tile_copy(shift)
        stride, toff = self.stride(scale), self.tile_offsets(shift)
        tiles = range(len(toff) - 1) if tiles is None else tiles
        edges = np.arange(stride, dtype=np.float64) / float(scale)
        lut = np.empty((len(tiles), stride), np.uint32)
        for k, t in enumerate(tiles):
            mz = copy["fragment_mz"][toff[t]:toff[t + 1]].astype(np.float64)
            row = toff[t] + np.searchsorted(mz, edges, side="left")
            row[0], row[-1] = toff[t], toff[t + 1]
            lut[k] = row
        return lut

    def pep_lut(self):
        """(bins, inv_w, table[bins + 1]); no table: (0, 0.0, empty)"""
        none = (0, F32(0.0), np.zeros(0, np.uint32))
        if self.np == 0:
            return none
        top = self.pep_mono[-1]
        if not (top >= F32(0.0)) or not (top < F32(1.0e30)):
            return none
        inv_w = F32(128.0)
        while float(top) * float(inv_w) + 2.0 > 4194304.0:
            inv_w = F32(inv_w * F32(0.5))
        bins = int(np.floor(float(top) * float(inv_w))) + 1
        edges = (np.arange(bins + 1, dtype=np.float64) / float(inv_w)).astype(F32)
        keys = np.sort(total_order_key(self.pep_mono))
        return bins, inv_w, np.searchsorted(keys, total_order_key(edges), side="left").astype(np.uint32)


def succinct(lut):
    """A row-major table [n_tiles, stride] in succinct form: (words, l1 [n_tiles * words] of (bits, rank), pos)."""
    n_tiles, stride = lut.shape
    words = (stride + 31) // 32
    occupied = np.zeros((n_tiles, words * 32), bool)
    occupied[:, :stride - 1] = lut[:, 1:] != lut[:, :-1]  # bit c: row[c + 1] != row[c], c + 1 < stride
    bits = np.packbits(occupied, axis=1, bitorder="little").view("<u4")  # [n_tiles, words]: bit b of word w is cell 32 w + b
    counts = popcount32(bits).astype(np.int64)
    counts[:, -1] += 1  # the slot of the tile's end, after the tile's last word
    flat = counts.reshape(-1)
    rank = np.cumsum(flat) - flat
    assert int(flat.sum()) < 1 << 32
    l1 = np.zeros(n_tiles * words, dtype=L.LUT_WORD_DTYPE)
    l1["bits"] = bits.reshape(-1)
    l1["rank"] = rank.astype(np.uint32)
    pos = np.concatenate([np.concatenate([lut[t, :stride - 1][occupied[t, :stride - 1]], lut[t, -1:]]) for t in range(n_tiles)])
    return words, l1, pos.astype(np.uint32)


def decode(l1, pos, n_tiles, stride):
    """The row-major table a succinct one stands for: pos[rank(c)] for every cell of every tile, with
    rank(c) = l1[c >> 5].rank + popcount(l1[c >> 5].bits & ((1 << (c & 31)) - 1))."""
    words = (stride + 31) // 32
    w = l1.reshape(n_tiles, words)
    c = np.arange(stride)
    bits, rank = np.repeat(w["bits"], 32, axis=1)[:, :stride], np.repeat(w["rank"], 32, axis=1)[:, :stride]  # of word c >> 5
    below = bits & ((np.uint32(1) << (c & 31).astype(np.uint32)) - np.uint32(1))
    return pos[rank.astype(np.int64) + popcount32(below)]
