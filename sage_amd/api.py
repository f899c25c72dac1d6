"""Host-side mirror of the sage-core API for the search-and-score path, over the C ABI.

Names and argument meaning follow the reference (crates/sage/src):
  DatabaseParameters  ~ database.rs:59-139   Builder / Parameters (JSON `database` section)
  IndexedDatabase     ~ database.rs:384-395
  SpectrumProcessor   ~ spectrum.rs:263-413
  Scorer              ~ scoring.rs:210-309
All compute happens in libsage_hip.so; nothing here falls back to Python arithmetic.
"""
import ctypes as C
import weakref
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


@dataclass
class Tolerance:  # mass.rs:10-16
    kind: str  # "ppm" | "pct" | "da"
    lo: float
    hi: float

    @staticmethod
    def from_json(obj) -> "Tolerance":
        (k, v), = obj.items()
        return Tolerance(k, float(v[0]), float(v[1]))

    def to_c(self):
        return L.SageTolerance(L.TOL_KINDS[self.kind], self.lo, self.hi)


@dataclass
class DatabaseParameters:
    """database.rs:59-93 Builder: None == field absent from the JSON."""
    bucket_size: Optional[int] = None
    enzyme: Optional[dict] = None  # keys: missed_cleavages,min_len,max_len,cleave_at,restrict,c_terminal,semi_enzymatic
    peptide_min_mass: Optional[float] = None
    peptide_max_mass: Optional[float] = None
    ion_kinds: Optional[List[str]] = None
    min_ion_index: Optional[int] = None
    static_mods: Optional[Dict[str, float]] = None
    variable_mods: Optional[Dict[str, List[float]]] = None
    max_variable_mods: Optional[int] = None
    decoy_tag: Optional[str] = None
    generate_decoys: Optional[bool] = None
    fasta: Optional[str] = None
    prefilter: Optional[bool] = None             # database.rs:88-92: search the FASTA in chunks first (runner.rs:104-127)
    prefilter_chunk_size: Optional[int] = None   # target proteins per chunk; None / 0 = auto (database.rs:142-160)
    prefilter_low_memory: Optional[bool] = None  # default true (database.rs:113)
    peptides_only: bool = False  # ours: stop after reorder_peptides; the fragment index is then built on the device

    @staticmethod
    def from_json(obj: dict) -> "DatabaseParameters":
        known = DatabaseParameters.__dataclass_fields__.keys()
        return DatabaseParameters(**{k: v for k, v in obj.items() if k in known})  # unknown keys ignored (serde)

    def to_c(self, struct_type=L.SageDbParams):
        """Builder::make_parameters defaults (database.rs:96-115).  Returns (struct, keepalive)."""
        keep = []
        p = struct_type()
        p.bucket_size = self.bucket_size if self.bucket_size is not None else 8192
        e = self.enzyme
        p.enzyme_present = 0 if e is None else 1
        e = e or {}

        def opt_int(key):
            v = e.get(key)
            return -1 if v is None else int(v)

        def opt_str(key):
            v = e.get(key)
            if v is None:
                return None
            b = v.encode()
            keep.append(b)
            return b

        p.missed_cleavages = opt_int("missed_cleavages")
        p.min_len = opt_int("min_len")
        p.max_len = opt_int("max_len")
        p.cleave_at = opt_str("cleave_at")
        p.restrict_ = opt_str("restrict")
        p.c_terminal = opt_int("c_terminal")
        p.semi_enzymatic = opt_int("semi_enzymatic")
        p.peptide_min_mass = 500.0 if self.peptide_min_mass is None else self.peptide_min_mass
        p.peptide_max_mass = 5000.0 if self.peptide_max_mass is None else self.peptide_max_mass
        kinds = np.array([L.ION_KINDS[k] for k in (self.ion_kinds if self.ion_kinds is not None else ["b", "y"])],
                         dtype=np.uint8)
        keep.append(kinds)
        p.ion_kinds = L.as_ptr(kinds, C.c_uint8)
        p.n_ion_kinds = len(kinds)
        p.min_ion_index = 2 if self.min_ion_index is None else self.min_ion_index
        sm = list((self.static_mods or {}).items())
        sk = (C.c_char_p * max(len(sm), 1))(*[k.encode() for k, _ in sm])
        sv = np.array([v for _, v in sm], dtype=np.float32)
        keep += [sk, sv]
        p.static_mod_keys = sk
        p.static_mod_masses = L.as_ptr(sv, C.c_float)
        p.n_static_mods = len(sm)
        vm = [(k, m) for k, ms in (self.variable_mods or {}).items()
              for m in (ms if isinstance(ms, (list, tuple)) else [ms])]
        vk = (C.c_char_p * max(len(vm), 1))(*[k.encode() for k, _ in vm])
        vv = np.array([m for _, m in vm], dtype=np.float32)
        keep += [vk, vv]
        p.var_mod_keys = vk
        p.var_mod_masses = L.as_ptr(vv, C.c_float)
        p.n_var_mods = len(vm)
        p.max_variable_mods = 2 if self.max_variable_mods is None else max(int(self.max_variable_mods), 1)
        tag = (self.decoy_tag if self.decoy_tag is not None else "rev_").encode()
        keep.append(tag)
        p.decoy_tag = tag
        p.generate_decoys = 1 if (self.generate_decoys is None or self.generate_decoys) else 0
        p.peptides_only = int(self.peptides_only)
        return p, keep

    def build(self, fasta_text: str, peptides_only: Optional[bool] = None) -> "IndexedDatabase":
        """Parameters::build(Fasta::parse(..)) — database.rs:260-263.  peptides_only: digest / modify / sort / dedup on the
        host and leave build_from_peptides (fragments, sort) to DeviceDatabase (index_build.hip)."""
        lib = L.load()
        p, keep = self.to_c()
        if peptides_only is not None:
            p.peptides_only = int(peptides_only)
        h = C.c_void_p()
        L.check(lib.sage_hip_hostdb_build(fasta_text.encode(), C.byref(p), C.byref(h)))
        return IndexedDatabase(h)

    # ---- the `prefilter` flow of sage-cli (runner.rs:104-127, :143-238) ----
    def num_targets(self, fasta_text: str) -> int:
        """Fasta::parse(..).targets.len()"""
        p, keep = self.to_c()
        n = C.c_uint64()
        L.check(L.load().sage_hip_fasta_num_targets(fasta_text.encode(), C.byref(p), C.byref(n)))
        return int(n.value)

    def auto_prefilter_chunk_size(self, fasta_text: str) -> int:
        """Parameters::auto_calculate_prefilter_chunk_size (database.rs:142-160)"""
        p, keep = self.to_c()
        n = C.c_uint64()
        L.check(L.load().sage_hip_prefilter_chunk_size(fasta_text.encode(), C.byref(p), int(self.prefilter_chunk_size or 0),
                                                       C.byref(n)))
        return int(n.value)

    def build_chunk(self, fasta_text: str, first_target: int, n_targets: int, peptides_only: Optional[bool] = None):
        """Parameters::build over one chunk of Fasta::iter_chunks (fasta.rs:81-89)"""
        p, keep = self.to_c()
        if peptides_only is not None:
            p.peptides_only = int(peptides_only)
        h = C.c_void_p()
        L.check(L.load().sage_hip_hostdb_build_chunk(fasta_text.encode(), C.byref(p), first_target, n_targets, C.byref(h)))
        return IndexedDatabase(h)

    def merge_kept(self, chunks, keeps, peptides_only: Optional[bool] = None) -> "IndexedDatabase":
        """runner.rs:215-238: the peptides quick_score kept in every chunk database -> reorder_peptides -> build_from_peptides"""
        p, keep = self.to_c()
        if peptides_only is not None:
            p.peptides_only = int(peptides_only)
        masks = [np.ascontiguousarray(k, dtype=np.uint8) for k in keeps]
        assert all(len(m) == c.n_peptides for m, c in zip(masks, chunks))
        hs = (C.c_void_p * max(len(chunks), 1))(*[c._h for c in chunks])
        ms = (L.c_u8_p * max(len(chunks), 1))(*[L.as_ptr(m, C.c_uint8) for m in masks])
        h = C.c_void_p()
        L.check(L.load().sage_hip_hostdb_merge_kept(hs, ms, len(chunks), C.byref(p), C.byref(h)))
        return IndexedDatabase(h)


def _view_array(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(C.addressof(ptr.contents))
    return np.frombuffer(buf, dtype=dtype, count=n)


class IndexedDatabase:
    """database.rs:384-395 — flat views over the host index built by libsage_hip."""

    def __init__(self, handle):
        self._h = handle
        lib = L.load()
        v = L.SageDbView()
        L.check(lib.sage_hip_hostdb_view(self._h, C.byref(v)))
        self._view = v
        self.n_peptides = int(v.n_peptides)
        self.n_fragments = int(v.n_fragments)
        self.bucket_size = int(v.bucket_size)
        self.has_fragments = bool(v.fragments)
        self.fragments = _view_array(v.fragments, self.n_fragments, L.THEORETICAL_DTYPE) if self.has_fragments else \
            np.zeros(0, dtype=L.THEORETICAL_DTYPE)
        self.min_value = _view_array(v.min_value, int(v.n_buckets), np.float32)
        self.pep_mono = _view_array(v.pep_mono, self.n_peptides, np.float32)
        self.seq_off = _view_array(v.seq_off, self.n_peptides + 1, np.uint64)
        total = int(self.seq_off[-1]) if self.n_peptides else 0
        self.seq = _view_array(v.seq, total, np.uint8)
        self.mods = _view_array(v.mods, total, np.float32)
        self.nterm = _view_array(v.nterm, self.n_peptides, np.float32)
        self.cterm = _view_array(v.cterm, self.n_peptides, np.float32)
        self.decoy = _view_array(v.decoy, self.n_peptides, np.uint8)
        self.missed_cleavages = _view_array(v.missed_cleavages, self.n_peptides, np.uint8)
        self.ion_kinds = _view_array(v.ion_kinds, int(v.n_ion_kinds), np.uint8)

    def size(self):  # database.rs:427-429
        return self.n_fragments

    def buckets(self):  # database.rs:431-433
        return self.min_value

    def peptide_string(self, i: int) -> str:
        lib = L.load()
        n = lib.sage_hip_hostdb_peptide_string(self._h, i, None, 0)
        buf = C.create_string_buffer(int(n))
        lib.sage_hip_hostdb_peptide_string(self._h, i, buf, n)
        return buf.value.decode()

    def peptide_proteins(self, i: int) -> str:
        lib = L.load()
        n = lib.sage_hip_hostdb_peptide_proteins(self._h, i, None, 0)
        buf = C.create_string_buffer(int(n))
        lib.sage_hip_hostdb_peptide_proteins(self._h, i, buf, n)
        return buf.value.decode()

    def protein_name(self, i: int) -> str:
        """name of protein `i` of the database (the FASTA accession, without the decoy tag)"""
        lib = L.load()
        n = lib.sage_hip_hostdb_protein_name(self._h, i, None, 0)
        if n == 0:
            raise IndexError(i)
        buf = C.create_string_buffer(int(n))
        lib.sage_hip_hostdb_protein_name(self._h, i, buf, n)
        return buf.value.decode()

    def group_graph(self, peptides) -> "GroupGraph":
        """ProteinGrouper::build (protein_grouping.rs:171-231) for the ascending, distinct peptide indices `peptides`: the host
        half of a grouping pass, without a device."""
        idx = np.ascontiguousarray(peptides, dtype=np.uint32)
        lib = L.load()
        h = C.c_void_p()
        L.check(lib.sage_hip_group_graph_build(self._h, L.as_ptr(idx, C.c_uint32), len(idx), C.byref(h)))
        try:
            v = L.SageGroupGraphView()
            L.check(lib.sage_hip_group_graph_view(h, C.byref(v)))
            ng, npr, ne = int(v.n_groups), int(v.n_proteins), int(v.n_edges)
            copy = lambda p, n, dt: _view_array(p, n, dt).copy() if n else np.zeros(0, dt)
            group_off = copy(v.group_off, ng + 1 if ng else 0, np.uint64)
            evidence_off = copy(v.evidence_off, ng + 1 if ng else 0, np.uint64)
            return GroupGraph(protein_id=copy(v.protein_id, npr, np.uint32), protein_decoy=copy(v.protein_decoy, npr, np.uint8),
                              n_meta_peptides=int(v.n_meta_peptides), group_off=group_off,
                              group_proteins=copy(v.group_proteins, int(group_off[-1]) if ng else 0, np.uint32),
                              evidence_off=evidence_off, evidence=copy(v.evidence, int(evidence_off[-1]) if ng else 0, np.uint32),
                              edge_group=copy(v.edge_group, ne, np.uint32), edge_meta=copy(v.edge_meta, ne, np.uint32))
        finally:
            lib.sage_hip_group_graph_free(h)

    def peptide_info(self, i: int):
        """(Peptide.proteins.len(), Peptide.semi_enzymatic)"""
        n, semi = C.c_uint32(), C.c_uint8()
        L.check(L.load().sage_hip_hostdb_peptide_info(self._h, i, C.byref(n), C.byref(semi)))
        return int(n.value), int(semi.value)

    def competition_keys(self, peptide_idx):
        """Map keys of fdr::picked_peptide / picked_protein (fdr.rs:126-132, :158-161) for PSMs of the given peptides:
        (peptide_key[n], n_peptide_keys, protein_key[n], n_protein_keys), dense ids, 0xFFFFFFFF = shared peptide."""
        idx = np.ascontiguousarray(peptide_idx, dtype=np.uint32)
        pk, prk = np.empty(len(idx), np.uint32), np.empty(len(idx), np.uint32)
        npk, nprk = C.c_uint32(), C.c_uint32()
        L.check(L.load().sage_hip_hostdb_competition_keys(self._h, L.as_ptr(idx, C.c_uint32), len(idx), L.as_ptr(pk, C.c_uint32),
                                                          C.byref(npk), L.as_ptr(prk, C.c_uint32), C.byref(nprk)))
        return pk, int(npk.value), prk, int(nprk.value)

    def isomer_groups(self):
        """Positional isomers: peptides with the same decoy flag, residues and multiset of modification masses.
        Returns (group_of[n_peptides] u32, 0xFFFFFFFF = no isomer; group_off[n_groups + 1] u64 into members; members u32):
        groups by ascending smallest member, members ascending."""
        lib = L.load()
        ng, nm = C.c_uint64(), C.c_uint64()
        group_of = np.empty(self.n_peptides, dtype=np.uint32)
        L.check(lib.sage_hip_hostdb_isomer_groups(self._h, L.as_ptr(group_of, C.c_uint32), None, None, C.byref(ng), C.byref(nm)))
        group_off = np.zeros(int(ng.value) + 1, dtype=np.uint64)
        members = np.zeros(max(int(nm.value), 1), dtype=np.uint32)
        L.check(lib.sage_hip_hostdb_isomer_groups(self._h, L.as_ptr(group_of, C.c_uint32), L.as_ptr(group_off, C.c_uint64),
                                                  L.as_ptr(members, C.c_uint32), C.byref(ng), C.byref(nm)))
        return group_of, group_off, members[:int(nm.value)]

    def feature_peptides(self, peptide_idx):
        """(seq_off[n + 1], residues, monoisotopic[n]) of the peptides behind `n` PSMs — the per-Feature peptide data the
        retention-time / mobility models embed (retention_model.rs:44-62, mobility_model.rs:103-158)."""
        idx = np.ascontiguousarray(peptide_idx, dtype=np.uint32)
        off = np.zeros(len(idx) + 1, dtype=np.uint64)
        lib = L.load()
        L.check(lib.sage_hip_hostdb_feature_peptides(self._h, L.as_ptr(idx, C.c_uint32), len(idx), L.as_ptr(off, C.c_uint64), None, None))
        seq = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
        mono = np.zeros(len(idx), dtype=np.float32)
        L.check(lib.sage_hip_hostdb_feature_peptides(self._h, L.as_ptr(idx, C.c_uint32), len(idx), L.as_ptr(off, C.c_uint64),
                                                     L.as_ptr(seq, C.c_uint8), L.as_ptr(mono, C.c_float)))
        return off, seq, mono

    def sequence(self, i: int) -> str:
        return bytes(self.seq[int(self.seq_off[i]):int(self.seq_off[i + 1])]).decode()

    def to_device(self, device: int = 0) -> "DeviceDatabase":
        return DeviceDatabase(self, device)

    def close(self):
        if self._h:
            L.load().sage_hip_hostdb_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceDatabase:
    def __init__(self, host, device: int = 0, build_on_device: bool = False):
        """host: an IndexedDatabase, or any object with a `_view` (L.SageDbView, whose arrays it keeps alive) and `has_fragments`.
        build_on_device: ignore the host's fragments (if any) and generate the index from the peptide list on the GPU
        (Parameters::build_from_peptides, database.rs:265-346); implied when the host database is peptides-only."""
        lib = L.load()
        self.host = host
        self.device = device
        self._h = C.c_void_p()
        view = host._view
        if build_on_device and host.has_fragments:
            view = L.SageDbView()
            C.memmove(C.byref(view), C.byref(host._view), C.sizeof(L.SageDbView))
            view.fragments = None
            view.n_fragments = 0
        L.check(lib.sage_hip_db_create(C.byref(view), device, C.byref(self._h)))
        self.device_bytes = int(lib.sage_hip_db_device_bytes(self._h))

    def layout(self) -> dict:
        """The scalars of the device layouts (sage_hip_debug_db_layout): tile shifts, table strides and scales, ..."""
        out = L.SageDbLayout()
        L.check(L.load().sage_hip_debug_db_layout(self._h, C.byref(out)))
        return {name: getattr(out, name) for name, _ in L.SageDbLayout._fields_}

    def table(self, name: str) -> np.ndarray:
        """One table of the device database copied back from HBM (sage_hip_debug_db_table; names: L.DB_TABLES).  "pm_frag" makes
        the peptide-major list again if the build released it."""
        table, dtype = L.DB_TABLES[name]
        lib = L.load()
        size = C.c_uint64()
        L.check(lib.sage_hip_debug_db_table(self._h, table, None, 0, C.byref(size)))
        assert size.value % dtype.itemsize == 0, (name, size.value)
        out = np.zeros(size.value // dtype.itemsize, dtype=dtype)
        if size.value:
            L.check(lib.sage_hip_debug_db_table(self._h, table, out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(size)))
            assert size.value == out.nbytes
        return out

    def close(self):
        if self._h:
            L.load().sage_hip_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class RawSpectrum:  # spectrum.rs:81-106 (MS2, centroided)
    mz: np.ndarray
    intensity: np.ndarray
    precursor_mz: float
    precursor_charge: Optional[int] = None
    isolation_window: Optional[Tuple[float, float]] = None  # Tolerance::Da(lo, hi)
    scan_start_time: float = 0.0
    inverse_ion_mobility: Optional[float] = None
    file_id: int = 0
    id: str = ""
    ion_injection_time: float = 0.0  # MS:1000927
    precursor_ref: str = ""          # precursors.first().spectrum_ref ("" == None)
    mobility: Optional[np.ndarray] = None  # per-peak ion mobility of an MS1 spectrum (spectrum.rs:344), None without one


@dataclass
class ProcessedSpectrum:  # spectrum.rs:57-79
    masses: np.ndarray
    intensities: np.ndarray
    total_ion_current: float
    precursor_mz: float
    precursor_charge: Optional[int] = None
    isolation_window: Optional[Tuple[float, float]] = None
    scan_start_time: float = 0.0
    inverse_ion_mobility: Optional[float] = None
    file_id: int = 0
    id: str = ""


class SpectrumProcessor:  # spectrum.rs:263-413
    def __init__(self, take_top_n: int, deisotope: bool, min_deisotope_mz: float = 0.0):
        self.take_top_n = take_top_n
        self.deisotope = deisotope
        self.min_deisotope_mz = min_deisotope_mz

    def process(self, raw: RawSpectrum) -> ProcessedSpectrum:
        lib = L.load()
        mz = np.ascontiguousarray(raw.mz, dtype=np.float32)
        it = np.ascontiguousarray(raw.intensity, dtype=np.float32)
        n = len(mz)
        om = np.empty(max(n, 1), dtype=np.float32)
        oi = np.empty(max(n, 1), dtype=np.float32)
        tic = C.c_float()
        k = lib.sage_hip_process_ms2(self.take_top_n, int(self.deisotope), self.min_deisotope_mz,
                                     L.as_ptr(mz, C.c_float), L.as_ptr(it, C.c_float), n,
                                     raw.precursor_charge or 0, L.as_ptr(om, C.c_float), L.as_ptr(oi, C.c_float),
                                     C.byref(tic))
        k = int(k)
        return ProcessedSpectrum(om[:k].copy(), oi[:k].copy(), float(np.float32(tic.value)), raw.precursor_mz,
                                 raw.precursor_charge, raw.isolation_window, raw.scan_start_time,
                                 raw.inverse_ion_mobility, raw.file_id, raw.id)


class SpectrumBatch:
    """SoA batch of ProcessedSpectrum (SageSpectrumBatch)."""

    def __init__(self, peak_off, masses, intensities, precursor_mz, precursor_charge, total_ion_current,
                 isolation_lo=None, isolation_hi=None, scan_start_time=None, inverse_ion_mobility=None, file_id=None):
        self.peak_off = np.ascontiguousarray(peak_off, dtype=np.uint64)
        self.masses = np.ascontiguousarray(masses, dtype=np.float32)
        self.intensities = np.ascontiguousarray(intensities, dtype=np.float32)
        self.precursor_mz = np.ascontiguousarray(precursor_mz, dtype=np.float32)
        self.precursor_charge = np.ascontiguousarray(precursor_charge, dtype=np.uint8)
        self.total_ion_current = np.ascontiguousarray(total_ion_current, dtype=np.float32)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        self.isolation_lo, self.isolation_hi = f32(isolation_lo), f32(isolation_hi)
        self.scan_start_time, self.inverse_ion_mobility = f32(scan_start_time), f32(inverse_ion_mobility)
        self.file_id = None if file_id is None else np.ascontiguousarray(file_id, dtype=np.uint32)
        self.n = len(self.precursor_mz)
        assert len(self.peak_off) == self.n + 1

    @staticmethod
    def from_spectra(spectra: Sequence[ProcessedSpectrum]) -> "SpectrumBatch":
        n = len(spectra)
        off = np.zeros(n + 1, dtype=np.uint64)
        for i, s in enumerate(spectra):
            off[i + 1] = off[i] + len(s.masses)
        cat = lambda xs: np.concatenate(xs).astype(np.float32) if n else np.zeros(0, np.float32)
        nan = float("nan")
        iso = [s.isolation_window for s in spectra]
        return SpectrumBatch(
            off, cat([s.masses for s in spectra]), cat([s.intensities for s in spectra]),
            [s.precursor_mz for s in spectra], [s.precursor_charge or 0 for s in spectra],
            [s.total_ion_current for s in spectra],
            [w[0] if w else nan for w in iso], [w[1] if w else nan for w in iso],
            [s.scan_start_time for s in spectra],
            [nan if s.inverse_ion_mobility is None else s.inverse_ion_mobility for s in spectra],
            [s.file_id for s in spectra])

    def page_locked(self) -> "SpectrumBatch":
        """The same batch with every array in page-locked host memory (sage_hip_host_alloc): Scorer.score then moves the
        peaks by DMA straight out of these arrays instead of staging them.  What a caller that owns its spectrum arena
        (the mzML reader, a Rust Vec allocated through the C ABI) would hand over."""
        lib = L.load()

        def lock(a):
            if a is None:
                return None
            # the block lives exactly as long as something refers to the array made over it (a view, a to_c() struct holding
            # the array, this batch): the ctypes buffer is the ndarray's base, and its finalizer frees the block
            p = C.c_void_p()
            L.check(lib.sage_hip_host_alloc(max(a.nbytes, 1), C.byref(p)))
            buf = (C.c_char * max(a.nbytes, 1)).from_address(p.value)
            weakref.finalize(buf, lib.sage_hip_host_free, C.c_void_p(p.value))
            out = np.frombuffer(buf, dtype=a.dtype, count=a.size).reshape(a.shape)
            out[...] = a
            return out

        b = SpectrumBatch.__new__(SpectrumBatch)
        for k in ("peak_off", "masses", "intensities", "precursor_mz", "precursor_charge", "total_ion_current", "isolation_lo",
                  "isolation_hi", "scan_start_time", "inverse_ion_mobility", "file_id"):
            setattr(b, k, lock(getattr(self, k)))
        b.n = self.n
        return b

    def subset(self, idx) -> "SpectrumBatch":
        idx = np.asarray(idx)
        lens = (self.peak_off[1:] - self.peak_off[:-1])[idx].astype(np.int64)
        off = np.zeros(len(idx) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        starts = self.peak_off[:-1][idx].astype(np.int64)
        gather = (np.repeat(starts - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]))) if len(idx) else np.zeros(0, np.int64)
        pick = lambda a: None if a is None else a[idx]
        return SpectrumBatch(off, self.masses[gather], self.intensities[gather], self.precursor_mz[idx],
                             self.precursor_charge[idx], self.total_ion_current[idx], pick(self.isolation_lo),
                             pick(self.isolation_hi), pick(self.scan_start_time), pick(self.inverse_ion_mobility),
                             pick(self.file_id))

    def to_c(self, struct_type=L.SageSpectrumBatch):
        b = struct_type()
        b.n_spectra = self.n
        p = lambda a, t: None if a is None else L.as_ptr(a, t)
        b.peak_off = p(self.peak_off, C.c_uint64)
        b.masses = p(self.masses, C.c_float)
        b.intensities = p(self.intensities, C.c_float)
        b.precursor_mz = p(self.precursor_mz, C.c_float)
        b.precursor_charge = p(self.precursor_charge, C.c_uint8)
        b.isolation_lo = p(self.isolation_lo, C.c_float)
        b.isolation_hi = p(self.isolation_hi, C.c_float)
        b.total_ion_current = p(self.total_ion_current, C.c_float)
        b.scan_start_time = p(self.scan_start_time, C.c_float)
        b.inverse_ion_mobility = p(self.inverse_ion_mobility, C.c_float)
        b.file_id = p(self.file_id, C.c_uint32)
        return b


@dataclass
class ScorerParams:
    """scoring.rs:210-232 Scorer fields (minus db); defaults = sage-cli input.rs:355-385."""
    precursor_tol: Tolerance = field(default_factory=lambda: Tolerance("ppm", -10.0, 10.0))
    fragment_tol: Tolerance = field(default_factory=lambda: Tolerance("ppm", -10.0, 10.0))
    min_matched_peaks: int = 4
    min_isotope_err: int = 0
    max_isotope_err: int = 0
    min_precursor_charge: int = 2
    max_precursor_charge: int = 4
    override_precursor_charge: bool = False
    max_fragment_charge: Optional[int] = None
    chimera: bool = False
    report_psms: int = 1
    wide_window: bool = False
    annotate_matches: bool = False
    score_type: str = "SageHyperScore"

    def to_c(self, struct_type=L.SageScorerParams):
        p = struct_type()
        p.precursor_tol = self.precursor_tol.to_c()
        p.fragment_tol = self.fragment_tol.to_c()
        p.min_matched_peaks = self.min_matched_peaks
        p.min_isotope_err = self.min_isotope_err
        p.max_isotope_err = self.max_isotope_err
        p.min_precursor_charge = self.min_precursor_charge
        p.max_precursor_charge = self.max_precursor_charge
        p.override_precursor_charge = int(self.override_precursor_charge)
        p.chimera = int(self.chimera)
        p.max_fragment_charge = -1 if self.max_fragment_charge is None else self.max_fragment_charge
        p.wide_window = int(self.wide_window)
        p.annotate_matches = int(self.annotate_matches)
        p.report_psms = self.report_psms
        p.score_type = L.SCORE_TYPES[self.score_type]
        return p


class RawBatch:
    """SoA batch of RawSpectrum (SageRawBatch): centroided MS2 peaks + precursors[0]."""

    def __init__(self, spectra: Sequence[RawSpectrum]):
        n = len(spectra)
        self.n = n
        self.ids = [s.id for s in spectra]
        self.peak_off = np.zeros(n + 1, dtype=np.uint64)
        for i, s in enumerate(spectra):
            self.peak_off[i + 1] = self.peak_off[i] + len(s.mz)
        cat = lambda xs: np.ascontiguousarray(np.concatenate(xs), dtype=np.float32) if n else np.zeros(0, np.float32)
        self.mz = cat([np.asarray(s.mz, np.float32) for s in spectra])
        self.intensities = cat([np.asarray(s.intensity, np.float32) for s in spectra])
        f32 = lambda xs: np.ascontiguousarray(xs, dtype=np.float32)
        nan = float("nan")
        self.precursor_mz = f32([s.precursor_mz for s in spectra])
        self.precursor_charge = np.ascontiguousarray([s.precursor_charge or 0 for s in spectra], dtype=np.uint8)
        self.isolation_lo = f32([s.isolation_window[0] if s.isolation_window else nan for s in spectra])
        self.isolation_hi = f32([s.isolation_window[1] if s.isolation_window else nan for s in spectra])
        self.scan_start_time = f32([s.scan_start_time for s in spectra])
        self.inverse_ion_mobility = f32([nan if s.inverse_ion_mobility is None else s.inverse_ion_mobility for s in spectra])
        self.file_id = np.ascontiguousarray([s.file_id for s in spectra], dtype=np.uint32)
        self.ion_injection_time = f32([s.ion_injection_time for s in spectra])
        self.precursor_ref = [s.precursor_ref for s in spectra]
        # per-peak ion mobility (MS1 only): None when no spectrum has one; else 0 inside the spectra without it
        self.mobility = self.has_mobility = None
        if any(s.mobility is not None for s in spectra):
            for s in spectra:
                if s.mobility is not None and len(s.mobility) != len(s.mz):
                    raise ValueError(f"spectrum {s.id!r}: {len(s.mobility)} mobilities for {len(s.mz)} peaks")
            self.mobility = cat([np.zeros(len(s.mz), np.float32) if s.mobility is None else np.asarray(s.mobility, np.float32)
                                 for s in spectra])
            self.has_mobility = np.ascontiguousarray([s.mobility is not None for s in spectra], dtype=np.uint8)

    @classmethod
    def from_arrays(cls, ids, peak_off, mz, intensities, precursor_mz, precursor_charge, isolation_lo, isolation_hi,
                    scan_start_time, inverse_ion_mobility, file_id, ion_injection_time=None, precursor_ref=None, mobility=None,
                    has_mobility=None) -> "RawBatch":
        """Adopt SoA arrays (NaN == None for the optional floats, 0 == unknown charge): what the C++ mzML reader returns.
        ion_injection_time / precursor_ref default to 0.0 / "".  mobility: per peak, like mz (MS1), or None; has_mobility: per
        spectrum (None with a mobility array: every spectrum has one)."""
        b = cls.__new__(cls)
        b.n = len(precursor_mz)
        b.ids = list(ids)
        b.peak_off = np.ascontiguousarray(peak_off, dtype=np.uint64)
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        b.mz, b.intensities = f32(mz), f32(intensities)
        b.precursor_mz = f32(precursor_mz)
        b.precursor_charge = np.ascontiguousarray(precursor_charge, dtype=np.uint8)
        b.isolation_lo, b.isolation_hi = f32(isolation_lo), f32(isolation_hi)
        b.scan_start_time, b.inverse_ion_mobility = f32(scan_start_time), f32(inverse_ion_mobility)
        b.file_id = np.ascontiguousarray(file_id, dtype=np.uint32)
        b.ion_injection_time = np.zeros(b.n, np.float32) if ion_injection_time is None else f32(ion_injection_time)
        b.precursor_ref = [""] * b.n if precursor_ref is None else list(precursor_ref)
        assert len(b.peak_off) == b.n + 1 and len(b.mz) == len(b.intensities) == int(b.peak_off[-1])
        b.mobility = b.has_mobility = None
        if mobility is not None:
            b.mobility = f32(mobility)
            b.has_mobility = np.ones(b.n, np.uint8) if has_mobility is None else np.ascontiguousarray(has_mobility, dtype=np.uint8)
            assert len(b.mobility) == len(b.mz) and len(b.has_mobility) == b.n
        return b

    def slice(self, begin: int, end: int) -> "RawBatch":
        """Spectra [begin, end) as a batch of their own (contiguous shard of a file)."""
        a, b = int(self.peak_off[begin]), int(self.peak_off[end])
        return RawBatch.from_arrays(self.ids[begin:end], self.peak_off[begin:end + 1] - np.uint64(a), self.mz[a:b], self.intensities[a:b],
                                    self.precursor_mz[begin:end], self.precursor_charge[begin:end], self.isolation_lo[begin:end],
                                    self.isolation_hi[begin:end], self.scan_start_time[begin:end],
                                    self.inverse_ion_mobility[begin:end], self.file_id[begin:end],
                                    self.ion_injection_time[begin:end], self.precursor_ref[begin:end],
                                    None if self.mobility is None else self.mobility[a:b],
                                    None if self.mobility is None else self.has_mobility[begin:end])

    def subset(self, idx) -> "RawBatch":
        """The spectra at positions `idx` as a batch of their own (a shard that is not contiguous in the file: sharding.plan_mass_shards)."""
        idx = np.asarray(idx, dtype=np.int64)
        lens = (self.peak_off[1:] - self.peak_off[:-1])[idx].astype(np.int64)
        off = np.zeros(len(idx) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        starts = self.peak_off[:-1][idx].astype(np.int64)
        gather = (np.repeat(starts - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]))) if len(idx) else np.zeros(0, np.int64)
        return RawBatch.from_arrays([self.ids[i] for i in idx], off, self.mz[gather], self.intensities[gather], self.precursor_mz[idx],
                                    self.precursor_charge[idx], self.isolation_lo[idx], self.isolation_hi[idx], self.scan_start_time[idx],
                                    self.inverse_ion_mobility[idx], self.file_id[idx], self.ion_injection_time[idx],
                                    [self.precursor_ref[i] for i in idx],
                                    None if self.mobility is None else self.mobility[gather],
                                    None if self.mobility is None else self.has_mobility[idx])

    def spectrum(self, i: int) -> RawSpectrum:
        lo, hi = int(self.peak_off[i]), int(self.peak_off[i + 1])
        iso = None if np.isnan(self.isolation_lo[i]) else (float(self.isolation_lo[i]), float(self.isolation_hi[i]))
        ims = None if np.isnan(self.inverse_ion_mobility[i]) else float(self.inverse_ion_mobility[i])
        return RawSpectrum(self.mz[lo:hi], self.intensities[lo:hi], float(self.precursor_mz[i]),
                           int(self.precursor_charge[i]) or None, iso, float(self.scan_start_time[i]), ims, int(self.file_id[i]),
                           self.ids[i], float(self.ion_injection_time[i]), self.precursor_ref[i],
                           self.mobility[lo:hi] if self.mobility is not None and self.has_mobility[i] else None)

    def to_c(self):
        b = L.SageRawBatch()
        b.n_spectra = self.n
        b.peak_off = L.as_ptr(self.peak_off, C.c_uint64)
        b.mz = L.as_ptr(self.mz, C.c_float)
        b.intensities = L.as_ptr(self.intensities, C.c_float)
        b.precursor_mz = L.as_ptr(self.precursor_mz, C.c_float)
        b.precursor_charge = L.as_ptr(self.precursor_charge, C.c_uint8)
        b.isolation_lo = L.as_ptr(self.isolation_lo, C.c_float)
        b.isolation_hi = L.as_ptr(self.isolation_hi, C.c_float)
        b.scan_start_time = L.as_ptr(self.scan_start_time, C.c_float)
        b.inverse_ion_mobility = L.as_ptr(self.inverse_ion_mobility, C.c_float)
        b.file_id = L.as_ptr(self.file_id, C.c_uint32)
        return b


def _kinds(iso_kind, n: int) -> np.ndarray:
    k = np.ascontiguousarray(iso_kind, dtype=np.uint8)
    if len(k) != n or (k > 2).any():
        raise ValueError("iso_kind: one Tolerance kind (0 ppm, 1 pct, 2 Da) per spectrum")
    return k if n else np.zeros(1, np.uint8)


class DeviceBatch:
    def __init__(self, scorer: "Scorer", batch: Optional[SpectrumBatch], handle=None, n: int = 0, iso_kind=None):
        lib = L.load()
        self._keep = batch
        if handle is not None:  # adopted (Scorer.process_upload)
            self._h, self.n = handle, n
            return
        self.n = batch.n
        self._h = C.c_void_p()
        cb = batch.to_c()
        if iso_kind is None:
            L.check(lib.sage_hip_batch_upload(scorer._h, C.byref(cb), C.byref(self._h)))
        else:
            kinds = _kinds(iso_kind, batch.n)
            L.check(lib.sage_hip_batch_upload_kinds(scorer._h, C.byref(cb), L.as_ptr(kinds, C.c_uint8), C.byref(self._h)))

    def download(self):
        """(peak_off[n+1], masses, intensities, total_ion_current[n]) of the resident ProcessedSpectrum arrays."""
        lib = L.load()
        off = np.zeros(self.n + 1, dtype=np.uint64)
        L.check(lib.sage_hip_batch_download(self._h, L.as_ptr(off, C.c_uint64), None, None, None))
        total = int(off[-1])
        m, it, tic = np.zeros(max(total, 1), np.float32), np.zeros(max(total, 1), np.float32), np.zeros(max(self.n, 1), np.float32)
        L.check(lib.sage_hip_batch_download(self._h, L.as_ptr(off, C.c_uint64), L.as_ptr(m, C.c_float), L.as_ptr(it, C.c_float),
                                            L.as_ptr(tic, C.c_float)))
        return off, m[:total], it[:total], tic[:self.n]

    def close(self):
        if self._h:
            L.load().sage_hip_batch_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ascore_from_counts(n=None, n_items=0, a=None, b=None, n_site_items=0):
    """The f64 arithmetic of site localisation on given integer counts, on the host (sage_hip_ascore_from_counts).
    n ([10]) with n_items -> depth_scores[10] and peptide_score; a, b ([10]) with n_site_items -> depth and ascore.  Returns a dict
    of what was asked for."""
    lib = L.load()
    out = {}
    n_p = a_p = b_p = ds_p = ps_p = d_p = as_p = None
    if n is not None:
        n = np.ascontiguousarray(n, dtype=np.uint16)
        if n.shape != (10,):
            raise ValueError("n needs 10 entries")
        ds, ps = np.zeros(10, dtype=np.float64), C.c_double()
        n_p, ds_p, ps_p = n.ctypes.data_as(C.c_void_p), ds.ctypes.data_as(C.c_void_p), C.cast(C.byref(ps), C.c_void_p)
    if a is not None or b is not None:
        a, b = np.ascontiguousarray(a, dtype=np.uint16), np.ascontiguousarray(b, dtype=np.uint16)
        if a.shape != (10,) or b.shape != (10,):
            raise ValueError("a and b need 10 entries each")
        depth, asc = C.c_uint8(), C.c_double()
        a_p, b_p = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
        d_p, as_p = C.cast(C.byref(depth), C.c_void_p), C.cast(C.byref(asc), C.c_void_p)
    L.check(lib.sage_hip_ascore_from_counts(n_p, int(n_items), a_p, b_p, int(n_site_items), ds_p, ps_p, d_p, as_p))
    if n is not None:
        out.update(depth_scores=ds, peptide_score=float(ps.value))
    if a is not None:
        out.update(depth=int(depth.value), ascore=float(asc.value))
    return out


class Scorer:
    """scoring.rs:210-309.  `score` takes a whole batch: a per-spectrum call cannot amortise a launch."""

    def __init__(self, db: DeviceDatabase, params: ScorerParams):
        lib = L.load()
        self.db = db
        self.params = params
        self._h = C.c_void_p()
        cp = params.to_c()
        L.check(lib.sage_hip_scorer_create(db._h, C.byref(cp), C.byref(self._h)))

    def clone(self) -> "Scorer":
        """A second handle on the same device database (own streams and working set): `&Scorer` is shared by every rayon
        worker in the reference (scoring.rs:300); calls on one handle serialise, clones run concurrently."""
        other = Scorer.__new__(Scorer)
        other.db, other.params, other._h = self.db, self.params, C.c_void_p()
        L.check(L.load().sage_hip_scorer_clone(self._h, C.byref(other._h)))
        return other

    def upload(self, batch: SpectrumBatch, iso_kind=None) -> DeviceBatch:
        """iso_kind: per-spectrum Tolerance kind of the isolation windows (0 ppm, 1 pct, 2 Da; None: all Da —
        sage_hip_batch_upload_kinds)"""
        return DeviceBatch(self, batch, iso_kind=iso_kind)

    def process_upload(self, raw: "RawBatch", take_top_n: int = 150, deisotope: bool = True, min_deisotope_mz: float = 0.0,
                       min_peaks: int = 15, iso_kind=None):
        """SpectrumProcessor::process (spectrum.rs:279-412) + the min_peaks filter of runner.rs:313 on the device; the
        processed batch stays resident.  Returns (DeviceBatch, peaks kept per spectrum before the filter).
        iso_kind: as for upload (sage_hip_batch_process_upload_kinds)."""
        lib = L.load()
        h = C.c_void_p()
        npk = np.zeros(max(raw.n, 1), dtype=np.uint32)
        cb = raw.to_c()
        if iso_kind is None:
            L.check(lib.sage_hip_batch_process_upload(self._h, C.byref(cb), take_top_n, int(deisotope), min_deisotope_mz, min_peaks,
                                                      C.byref(h), L.as_ptr(npk, C.c_uint32)))
        else:
            kinds = _kinds(iso_kind, raw.n)
            L.check(lib.sage_hip_batch_process_upload_kinds(self._h, C.byref(cb), L.as_ptr(kinds, C.c_uint8), take_top_n,
                                                            int(deisotope), min_deisotope_mz, min_peaks, C.byref(h),
                                                            L.as_ptr(npk, C.c_uint32)))
        return DeviceBatch(self, None, handle=h, n=raw.n), npk[:raw.n]

    def _alloc_out(self, n):
        """Output arrays in page-locked host memory (sage_hip_host_alloc), reused while the size is unchanged.
        NOTE: a later call with the same batch size overwrites the arrays returned by the previous one."""
        key = (n, self.params.report_psms)
        cached = getattr(self, "_pinned", None)
        if cached is None or cached[0] != key:
            self._free_pinned()
            lib = L.load()
            nb_f = max(n * self.params.report_psms, 1) * L.FEATURE_DTYPE.itemsize
            nb_c = max(n, 1) * 4
            pf, pc = C.c_void_p(), C.c_void_p()
            L.check(lib.sage_hip_host_alloc(nb_f, C.byref(pf)))
            L.check(lib.sage_hip_host_alloc(nb_c, C.byref(pc)))
            feats = np.frombuffer((C.c_char * nb_f).from_address(pf.value), dtype=L.FEATURE_DTYPE,
                                  count=n * self.params.report_psms)
            counts = np.frombuffer((C.c_char * nb_c).from_address(pc.value), dtype=np.uint32, count=n)
            self._pinned = (key, pf, pc, feats, counts)
        _, _, _, feats, counts = self._pinned
        return feats, counts

    def _free_pinned(self):
        cached = getattr(self, "_pinned", None)
        if cached is not None:
            lib = L.load()
            lib.sage_hip_host_free(cached[1])
            lib.sage_hip_host_free(cached[2])
            self._pinned = None

    def score_resident(self, dbatch: DeviceBatch):
        lib = L.load()
        feats, counts = self._alloc_out(dbatch.n)
        L.check(lib.sage_hip_score_resident(self._h, dbatch._h, feats.ctypes.data_as(C.c_void_p),
                                            L.as_ptr(counts, C.c_uint32)))
        return feats.reshape(dbatch.n, self.params.report_psms), counts

    def score(self, batch: SpectrumBatch, pinned_out: bool = True, iso_kind=None):
        """Vec<Feature> per spectrum: returns (features[n, report_psms], counts[n]).  Host arrays in, host arrays out, through
        the upload / score / download pipeline of sage_hip_score_batch.  pinned_out=False: plain (pageable) result arrays.
        iso_kind: as for upload (sage_hip_score_batch_kinds)."""
        lib = L.load()
        if pinned_out:
            feats, counts = self._alloc_out(batch.n)
        else:
            feats = np.zeros(batch.n * self.params.report_psms, dtype=L.FEATURE_DTYPE)
            counts = np.zeros(batch.n, dtype=np.uint32)
        cb = batch.to_c()
        if iso_kind is None:
            L.check(lib.sage_hip_score_batch(self._h, C.byref(cb), feats.ctypes.data_as(C.c_void_p),
                                             L.as_ptr(counts, C.c_uint32)))
        else:
            kinds = _kinds(iso_kind, batch.n)
            L.check(lib.sage_hip_score_batch_kinds(self._h, C.byref(cb), L.as_ptr(kinds, C.c_uint8), feats.ctypes.data_as(C.c_void_p),
                                                   L.as_ptr(counts, C.c_uint32)))
        return feats.reshape(batch.n, self.params.report_psms), counts

    def annotate(self, dbatch: DeviceBatch, feats: np.ndarray, counts: np.ndarray):
        """Fragments (scoring.rs:152-161) of the PSMs that score_resident returned for this batch (annotate_matches).
        Returns (psm_off[n * report_psms + 1], dict of flat arrays); PSM r of spectrum i is slot i * report_psms + r."""
        lib = L.load()
        rp = self.params.report_psms
        feats = np.ascontiguousarray(feats).reshape(dbatch.n * rp)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        valid = (np.arange(rp)[None, :] < counts[:, None]).reshape(-1)
        total = int(feats["matched_peaks"][valid].sum())
        off = np.zeros(dbatch.n * rp + 1, dtype=np.uint64)
        arr = dict(kinds=np.zeros(total, np.uint8), charges=np.zeros(total, np.int32), fragment_ordinals=np.zeros(total, np.int32),
                   intensities=np.zeros(total, np.float32), mz_calculated=np.zeros(total, np.float32),
                   mz_experimental=np.zeros(total, np.float32))
        fr = L.SageFragments(total, L.as_ptr(off, C.c_uint64), L.as_ptr(arr["kinds"], C.c_uint8),
                             arr["charges"].ctypes.data_as(C.POINTER(C.c_int32)),
                             arr["fragment_ordinals"].ctypes.data_as(C.POINTER(C.c_int32)),
                             L.as_ptr(arr["intensities"], C.c_float), L.as_ptr(arr["mz_calculated"], C.c_float),
                             L.as_ptr(arr["mz_experimental"], C.c_float))
        L.check(lib.sage_hip_annotate_resident(self._h, dbatch._h, feats.ctypes.data_as(C.c_void_p),
                                               L.as_ptr(counts, C.c_uint32), C.byref(fr)))
        return off, arr

    def score_candidates(self, dbatch: DeviceBatch, feats: np.ndarray, counts: np.ndarray, cand_off, cand_pep, cand_charge=None):
        """score_candidate (scoring.rs:675-767) of given peptides against the spectra of the PSMs that score_resident returned for
        this batch: PSM r of spectrum i is slot i * report_psms + r and gets the peptides cand_pep[cand_off[slot] : cand_off[slot + 1]],
        scored on the spectrum as PSM r saw it (chimera: after the peak removal of the ranks before it).  cand_charge: precursor
        charge per candidate (None or 0: the PSM's own).  Returns a structured array (L.CANDIDATE_SCORE_DTYPE), one per candidate."""
        lib = L.load()
        feats, counts, cand_off, cand_pep, cand_charge = self._candidate_lists(dbatch, feats, counts, cand_off, cand_pep, cand_charge)
        charge_p = None if cand_charge is None else L.as_ptr(cand_charge, C.c_uint8)
        out = np.zeros(int(cand_off[-1]) if len(cand_off) else 0, dtype=L.CANDIDATE_SCORE_DTYPE)
        L.check(lib.sage_hip_score_candidates_resident(self._h, dbatch._h, feats.ctypes.data_as(C.c_void_p), L.as_ptr(counts, C.c_uint32),
                                                       L.as_ptr(cand_off, C.c_uint64), L.as_ptr(cand_pep, C.c_uint32), charge_p,
                                                       out.ctypes.data_as(C.c_void_p)))
        return out

    def _candidate_lists(self, dbatch, feats, counts, cand_off, cand_pep, cand_charge):
        """the list arguments of score_candidates / localise, checked and made contiguous"""
        rp = self.params.report_psms
        feats = np.ascontiguousarray(feats).reshape(dbatch.n * rp)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        cand_off = np.ascontiguousarray(cand_off, dtype=np.uint64)
        cand_pep = np.ascontiguousarray(cand_pep, dtype=np.uint32)
        if len(cand_off) != dbatch.n * rp + 1 or len(counts) != dbatch.n:
            raise ValueError("cand_off needs n * report_psms + 1 entries, counts n")
        if len(cand_pep) < int(cand_off.max(initial=0)):
            raise ValueError("cand_off points behind cand_pep")
        if cand_charge is not None:
            if np.any((np.asarray(cand_charge) < 0) | (np.asarray(cand_charge) > 255)):
                raise ValueError("cand_charge outside 0..255")
            cand_charge = np.ascontiguousarray(cand_charge, dtype=np.uint8)
            if len(cand_charge) != len(cand_pep):
                raise ValueError("cand_charge and cand_pep differ in length")
        return feats, counts, cand_off, cand_pep, cand_charge

    def localise(self, dbatch: DeviceBatch, feats: np.ndarray, counts: np.ndarray, cand_off, cand_pep, cand_charge=None,
                 per_candidate: bool = False):
        """Site localisation over the lists score_candidates takes: per PSM slot the two candidates with the largest
        peptide score and the Ascore between them.  Returns a structured array (L.LOCALISATION_DTYPE) of n * report_psms slots —
        a slot without candidates has best == second == 0xFFFFFFFF and ascore NaN — and, with per_candidate, the depth counts of
        every candidate (L.DEPTH_COUNTS_DTYPE) as a second value."""
        lib = L.load()
        feats, counts, cand_off, cand_pep, cand_charge = self._candidate_lists(dbatch, feats, counts, cand_off, cand_pep, cand_charge)
        slots = np.zeros(dbatch.n * self.params.report_psms, dtype=L.LOCALISATION_DTYPE)
        slots["best"] = slots["second"] = 0xFFFFFFFF
        slots["ascore"] = np.nan
        total = int(cand_off[-1]) if len(cand_off) else 0
        cnt = np.zeros(total, dtype=L.DEPTH_COUNTS_DTYPE) if per_candidate else None
        L.check(lib.sage_hip_localise_resident(self._h, dbatch._h, feats.ctypes.data_as(C.c_void_p), L.as_ptr(counts, C.c_uint32),
                                               L.as_ptr(cand_off, C.c_uint64), L.as_ptr(cand_pep, C.c_uint32),
                                               None if cand_charge is None else L.as_ptr(cand_charge, C.c_uint8),
                                               cnt.ctypes.data_as(C.c_void_p) if per_candidate and total else None,
                                               slots.ctypes.data_as(C.c_void_p)))
        return (slots, cnt) if per_candidate else slots

    def last_localise_timing(self):
        """(ms of the last localise call on the scorer's stream, ms of its two kernels alone), from HIP events"""
        a, k = C.c_float(), C.c_float()
        L.check(L.load().sage_hip_last_localise_timing(self._h, C.byref(a), C.byref(k)))
        return float(a.value), float(k.value)

    def last_candidates_timing(self):
        """(ms of the last score_candidates call on the scorer's stream, ms of its kernel alone), from HIP events"""
        a, k = C.c_float(), C.c_float()
        L.check(L.load().sage_hip_last_candidates_timing(self._h, C.byref(a), C.byref(k)))
        return float(a.value), float(k.value)

    def quick_score(self, dbatch: DeviceBatch, prefilter_low_memory: bool, keep: Optional[np.ndarray] = None) -> np.ndarray:
        """Scorer::quick_score (scoring.rs:255-298) over the batch; `keep` ([n_peptides] u8) is OR-updated and returned."""
        lib = L.load()
        if keep is None:
            keep = np.zeros(self.db.host.n_peptides, dtype=np.uint8)
        assert keep.dtype == np.uint8 and len(keep) == self.db.host.n_peptides
        L.check(lib.sage_hip_quick_score_resident(self._h, dbatch._h, int(prefilter_low_memory), L.as_ptr(keep, C.c_uint8)))
        return keep

    def initial_hits(self, dbatch: DeviceBatch):
        lib = L.load()
        cap = max(50, 2 * self.params.report_psms)
        packed = np.zeros((dbatch.n, cap), dtype=np.uint64)
        ln = np.zeros(dbatch.n, dtype=np.uint32)
        mp = np.zeros(dbatch.n, dtype=np.uint64)
        sc = np.zeros(dbatch.n, dtype=np.uint64)
        L.check(lib.sage_hip_initial_hits(self._h, dbatch._h, L.as_ptr(packed, C.c_uint64), cap,
                                          L.as_ptr(ln, C.c_uint32), L.as_ptr(mp, C.c_uint64),
                                          L.as_ptr(sc, C.c_uint64)))
        return packed, ln, mp, sc

    def set_timing_interval(self, every: int):
        """Per-kernel HIP events on every `every`-th score_resident call only (0: never; default 1): sage_hip.h."""
        L.check(L.load().sage_hip_scorer_set_timing_interval(self._h, int(every)))

    def last_timing(self) -> dict:
        t = L.SageTiming()
        L.check(L.load().sage_hip_last_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in L.SageTiming._fields_}

    def close(self):
        if self._h:
            self._free_pinned()
            L.load().sage_hip_scorer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class RescoreResult:
    """Outputs of sage_hip_rescore, input order (Feature fields of scoring.rs:124-136) + the reference's output order."""
    discriminant_score: np.ndarray
    posterior_error: np.ndarray
    spectrum_q: np.ndarray
    peptide_q: np.ndarray
    protein_q: np.ndarray
    order: np.ndarray
    passing_spectrum: int
    passing_peptide: int
    passing_protein: int
    lda_fitted: bool
    coef: np.ndarray
    device_ms: float


def rescore(features: np.ndarray, precursor_tol: Tolerance, peptide_key, n_peptide_keys: int, protein_key,
            n_protein_keys: int, aligned_rt=None, delta_rt_model=None, delta_ims_model=None, device: int = 0) -> RescoreResult:
    """spectrum_fdr + picked_peptide + picked_protein (sage-cli runner.rs:536-541) over ALL Features of a run, on the
    device (rescore.hip).  `features`: 1-D array of FEATURE_DTYPE."""
    f = np.ascontiguousarray(features, dtype=L.FEATURE_DTYPE).reshape(-1)
    n = len(f)
    pk = np.ascontiguousarray(peptide_key, dtype=np.uint32)
    prk = np.ascontiguousarray(protein_key, dtype=np.uint32)
    assert len(pk) == n and len(prk) == n
    opt = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (aligned_rt, delta_rt_model, delta_ims_model)]
    outs = [np.empty(n, np.float32) for _ in range(5)]
    order = np.empty(n, np.uint32)
    cin = L.SageRescoreInput(n, f.ctypes.data, *[None if a is None else L.as_ptr(a, C.c_float) for a in opt],
                             precursor_tol.to_c(), L.as_ptr(pk, C.c_uint32), n_peptide_keys, L.as_ptr(prk, C.c_uint32),
                             n_protein_keys)
    cout = L.SageRescoreOutput(*[L.as_ptr(a, C.c_float) for a in outs], L.as_ptr(order, C.c_uint32))
    L.check(L.load().sage_hip_rescore(device, C.byref(cin), C.byref(cout)))
    return RescoreResult(*outs, order, int(cout.passing_spectrum), int(cout.passing_peptide), int(cout.passing_protein),
                         bool(cout.lda_fitted), np.array(cout.coef[:], dtype=np.float64), float(cout.device_ms))


@dataclass
class GroupGraph:
    """IndexedDatabase.group_graph: proteins in numbering order (ProteinIx -> a database protein with that name, decoy flag), the
    groups (ProteinIx lists), every group's evidence (ascending meta-peptide indices) and the edge list of the set cover."""
    protein_id: np.ndarray
    protein_decoy: np.ndarray
    n_meta_peptides: int
    group_off: np.ndarray
    group_proteins: np.ndarray
    evidence_off: np.ndarray
    evidence: np.ndarray
    edge_group: np.ndarray
    edge_meta: np.ndarray

    @property
    def n_groups(self) -> int:
        return max(len(self.group_off) - 1, 0)


@dataclass
class ProteinGroupResult:
    """Outputs of sage_hip_protein_groups, input order: Feature.protein_groups (strings[string_id[i]]), num_protein_groups,
    protein_group_q; the passing count of picked_protein_group and the sizes of the last pass's graph."""
    strings: List[str]
    string_id: np.ndarray
    num_protein_groups: np.ndarray
    protein_group_q: np.ndarray
    passing_protein_group: int
    n_groups: int
    n_meta_peptides: int
    cover_rounds: int
    device_ms: float
    host_graph_ms: float

    def protein_groups(self, i: int) -> str:
        return self.strings[int(self.string_id[i])]


def protein_groups(db: "IndexedDatabase", features: np.ndarray, peptide_q, discriminant_score, protein_grouping: bool = True,
                   peptide_fdr: float = 0.01, device: int = 0) -> ProteinGroupResult:
    """generate_protein_groups + picked_protein_group (sage-cli runner.rs:539-549) over ALL Features of a run: IDPicker protein
    groups in two passes, the fallback protein list, and the picked protein-group FDR, on the device (protein_groups.hip) with the
    graph and the strings built on the host (groups.cpp).  `features`: 1-D array of FEATURE_DTYPE."""
    f = np.ascontiguousarray(features, dtype=L.FEATURE_DTYPE).reshape(-1)
    n = len(f)
    pq = np.ascontiguousarray(peptide_q, dtype=np.float32)
    ds = np.ascontiguousarray(discriminant_score, dtype=np.float32)
    assert len(pq) == n and len(ds) == n
    num, sid, q = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.ones(n, np.float32)
    cin = L.SageGroupInput(n, f.ctypes.data, L.as_ptr(pq, C.c_float), L.as_ptr(ds, C.c_float), int(bool(protein_grouping)),
                           float(peptide_fdr))
    cout = L.SageGroupOutput(L.as_ptr(num, C.c_uint32), L.as_ptr(q, C.c_float), L.as_ptr(sid, C.c_uint32))
    lib = L.load()
    L.check(lib.sage_hip_protein_groups(device, db._h, C.byref(cin), C.byref(cout)))
    try:
        strings = [lib.sage_hip_group_string(cout.strings, i).decode() for i in range(int(cout.n_strings))]
    finally:
        lib.sage_hip_group_strings_free(cout.strings)
    return ProteinGroupResult(strings, sid, num, q, int(cout.passing_protein_group), int(cout.n_groups), int(cout.n_meta_peptides),
                              int(cout.cover_rounds), float(cout.device_ms), float(cout.host_graph_ms))


@dataclass
class RtPrediction:
    """Outputs of sage_hip_predict_rt, input order (Feature fields aligned_rt, predicted_rt, delta_rt_model, predicted_ims,
    delta_ims_model; spectrum_q of the poisson-sorted pass) + the per-file alignments."""
    spectrum_q: np.ndarray
    aligned_rt: np.ndarray
    predicted_rt: np.ndarray
    delta_rt_model: np.ndarray
    predicted_ims: np.ndarray
    delta_ims_model: np.ndarray
    alignments: np.ndarray  # [n_files] of (file_id, max_rt, slope, intercept)
    rt_fitted: bool
    ims_fitted: bool
    rt_r2: float
    ims_r2: float
    device_ms: float


ALIGNMENT_DTYPE = np.dtype([("file_id", "<u4"), ("max_rt", "<f4"), ("slope", "<f4"), ("intercept", "<f4")])


def predict_rt(features: np.ndarray, n_files: int, seq_off, seq, monoisotopic, device: int = 0) -> RtPrediction:
    """The predict_rt block of sage-cli (runner.rs:513-530) on the device: poisson-sorted q-values, global retention-time
    alignment, retention-time and ion-mobility linear models."""
    f = np.ascontiguousarray(features, dtype=L.FEATURE_DTYPE).reshape(-1)
    n = len(f)
    off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    sq = np.ascontiguousarray(seq, dtype=np.uint8)
    mono = np.ascontiguousarray(monoisotopic, dtype=np.float32)
    assert len(off) == n + 1 and len(mono) == n
    outs = [np.empty(n, np.float32) for _ in range(6)]
    al = np.zeros(n_files, dtype=ALIGNMENT_DTYPE)
    cin = L.SageRtInput(n, f.ctypes.data, n_files, L.as_ptr(off, C.c_uint64), L.as_ptr(sq, C.c_uint8), L.as_ptr(mono, C.c_float))
    cout = L.SageRtOutput(*[L.as_ptr(a, C.c_float) for a in outs], C.cast(al.ctypes.data, C.POINTER(L.SageAlignment)))
    L.check(L.load().sage_hip_predict_rt(device, C.byref(cin), C.byref(cout)))
    return RtPrediction(*outs, al, bool(cout.rt_fitted), bool(cout.ims_fitted), float(cout.rt_r2), float(cout.ims_r2),
                        float(cout.device_ms))


def device_count() -> int:
    return int(L.load().sage_hip_device_count())


# ---- label-free MS1 quantification (sage_hip_lfq) ---------------------------------------------------------------------------
LFQ_SCORING = ("RetentionTime", "SpectralAngle", "Intensity", "Hybrid")  # lfq.rs:25-31 PeakScoringStrategy
LFQ_INTEGRATION = ("Apex", "Sum")                                         # lfq.rs:33-37 IntegrationStrategy


@dataclass
class LfqSettings:  # lfq.rs:45-68 (defaults of LfqSettings::default)
    peak_scoring: str = "Hybrid"
    integration: str = "Sum"
    spectral_angle: float = 0.70
    ppm_tolerance: float = 5.0
    mobility_pct_tolerance: float = 1.0
    combine_charge_states: bool = True
    peptide_q_value: float = 0.01

    def to_c(self, precursor_charge) -> "L.SageLfqSettings":
        if self.peak_scoring not in LFQ_SCORING or self.integration not in LFQ_INTEGRATION:
            raise ValueError(f"unknown LFQ strategy {self.peak_scoring!r} / {self.integration!r}")
        return L.SageLfqSettings(LFQ_SCORING.index(self.peak_scoring), LFQ_INTEGRATION.index(self.integration),
                                 float(self.spectral_angle), float(self.ppm_tolerance), float(self.mobility_pct_tolerance),
                                 float(self.peptide_q_value), int(bool(self.combine_charge_states)), int(precursor_charge[0]),
                                 int(precursor_charge[1]), 0)


# mass.rs:78-104 composition(aa): carbon and sulfur atoms per residue
_CARBON = np.zeros(256, dtype=np.uint16)
_SULFUR = np.zeros(256, dtype=np.uint16)
for _aa, _c, _s in (("A", 3, 0), ("R", 6, 0), ("N", 4, 0), ("D", 4, 0), ("C", 3, 1), ("E", 5, 0), ("Q", 5, 0), ("G", 2, 0),
                    ("H", 6, 0), ("I", 6, 0), ("L", 6, 0), ("K", 6, 0), ("M", 5, 1), ("F", 9, 0), ("P", 5, 0), ("S", 3, 0),
                    ("T", 4, 0), ("W", 11, 0), ("Y", 9, 0), ("V", 5, 0), ("U", 3, 0), ("O", 12, 0)):
    _CARBON[ord(_aa)], _SULFUR[ord(_aa)] = _c, _s


def peptide_compositions(seq_off, seq):
    """(carbon[n], sulfur[n]) of every peptide: the Composition sum of lfq.rs:258-263 (u16)."""
    off = np.asarray(seq_off, dtype=np.int64)
    s = np.asarray(seq, dtype=np.uint8)
    n = len(off) - 1
    if n <= 0:
        return np.zeros(0, np.uint16), np.zeros(0, np.uint16)
    cs = np.concatenate([[0], np.cumsum(_CARBON[s].astype(np.int64))])
    ss = np.concatenate([[0], np.cumsum(_SULFUR[s].astype(np.int64))])
    return ((cs[off[1:]] - cs[off[:-1]]).astype(np.uint16), (ss[off[1:]] - ss[off[:-1]]).astype(np.uint16))


@dataclass
class LfqResult:
    """Grids of sage_hip_lfq in ascending (peptide_idx, charge, decoy) order; charge 0 when charge states are combined.
    areas / warps: [n, n_files]; matrix: [n, n_files * 3, 100] (debug=True) or None."""
    peptide_idx: np.ndarray
    charge: np.ndarray
    decoy: np.ndarray
    has_peak: np.ndarray
    peak_rt: np.ndarray
    left: np.ndarray
    right: np.ndarray
    score: np.ndarray
    spectral_angle: np.ndarray
    q_value: np.ndarray
    areas: np.ndarray
    warps: np.ndarray
    matrix: Optional[np.ndarray]
    n_windows: int
    n_contributions: int
    passing: int
    stage_ms: dict

    def target_rows(self) -> np.ndarray:
        """the rows lfq.tsv holds (runner.rs:1207-1210: targets; Traces::integrate returned a peak)"""
        return np.flatnonzero((self.decoy == 0) & (self.has_peak != 0)).astype(np.uint64)

    def to_c(self, keep: list) -> "L.SageLfqOutput":
        arr = lambda a, t: (keep.append(a), L.as_ptr(a, t))[1]
        return L.SageLfqOutput(len(self.peptide_idx), arr(self.peptide_idx, C.c_uint32), arr(self.charge, C.c_uint8),
                               arr(self.decoy, C.c_uint8), arr(self.has_peak, C.c_uint8), arr(self.peak_rt, C.c_uint32),
                               arr(self.left, C.c_uint32), arr(self.right, C.c_uint32), arr(self.score, C.c_double),
                               arr(self.spectral_angle, C.c_double), arr(self.q_value, C.c_float),
                               arr(np.ascontiguousarray(self.areas), C.c_double), None, None, len(self.peptide_idx))


def lfq(features: np.ndarray, order, aligned_rt, peptide_q, alignments: np.ndarray, ms1: Sequence[RawBatch], carbon, sulfur,
        settings: LfqSettings, precursor_charge, device: int = 0, debug: bool = False, ion_mobility: bool = False) -> LfqResult:
    """build_feature_map(..).quantify(..) + picked_precursor (sage-cli runner.rs:562-575) on the device.
    features / aligned_rt / peptide_q: the run's PSMs (input order) and their rescoring outputs; order: confidence order
    (RescoreResult.order) or None; alignments: RtPrediction.alignments; ms1: raw MS1 spectra (RawBatch per file, file_id set);
    carbon / sulfur: peptide_compositions of the database.  debug: also the warps and the grid matrices.
    ion_mobility: sage_hip_lfq_im (lfq_im) instead of sage_hip_lfq — the batches' per-peak mobility columns and the features'
    `ims` take part."""
    f = np.ascontiguousarray(features, dtype=L.FEATURE_DTYPE).reshape(-1)
    n = len(f)
    order_a = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    art = np.ascontiguousarray(aligned_rt, dtype=np.float32)
    pq = np.ascontiguousarray(peptide_q, dtype=np.float32)
    al = np.ascontiguousarray(alignments, dtype=ALIGNMENT_DTYPE)
    carbon = np.ascontiguousarray(carbon, dtype=np.uint16)
    sulfur = np.ascontiguousarray(sulfur, dtype=np.uint16)
    assert len(art) == n and len(pq) == n and (order_a is None or len(order_a) == n) and len(carbon) == len(sulfur)
    n_files = len(al)
    nz = int(precursor_charge[1]) - int(precursor_charge[0]) + 1
    cand = (pq <= np.float32(settings.peptide_q_value)) & (f["label"] == 1)
    cap = len(np.unique(f["peptide_idx"][cand])) * (2 if settings.combine_charge_states else 2 * nz)
    batches = [b.to_c() for b in ms1]
    cms1 = (L.SageRawBatch * max(len(batches), 1))(*batches)
    cin = L.SageLfqInput(n, f.ctypes.data, None if order_a is None else L.as_ptr(order_a, C.c_uint32), L.as_ptr(art, C.c_float),
                         L.as_ptr(pq, C.c_float), C.cast(al.ctypes.data, C.POINTER(L.SageAlignment)), n_files, len(batches), cms1,
                         len(carbon), L.as_ptr(carbon, C.c_uint16), L.as_ptr(sulfur, C.c_uint16), settings.to_c(precursor_charge))
    r = LfqResult(np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8),
                  np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.float64),
                  np.zeros(cap, np.float64), np.ones(cap, np.float32), np.zeros((cap, n_files), np.float64),
                  np.zeros((cap, n_files), np.int32), np.zeros((cap, n_files * 3, 100), np.float64) if debug else None, 0, 0, 0, {})
    keep = []
    cout = r.to_c(keep)
    cout.warps = L.as_ptr(r.warps, C.c_int32)
    if debug:
        cout.matrix = L.as_ptr(r.matrix, C.c_double)
    if ion_mobility:
        mob = (L.SageLfqMobility * max(len(ms1), 1))()
        for k, b in enumerate(ms1):
            if b.mobility is not None:
                mob[k].mobility = L.as_ptr(b.mobility, C.c_float)
                mob[k].has_mobility = L.as_ptr(b.has_mobility, C.c_uint8)
        L.check(L.load().sage_hip_lfq_im(device, C.byref(cin), mob, C.byref(cout)))
    else:
        L.check(L.load().sage_hip_lfq(device, C.byref(cin), C.byref(cout)))
    g = int(cout.n_grids)
    for k in ("peptide_idx", "charge", "decoy", "has_peak", "peak_rt", "left", "right", "score", "spectral_angle", "q_value",
              "areas", "warps", "matrix"):
        v = getattr(r, k)
        if v is not None:
            setattr(r, k, v[:g])
    r.n_windows, r.n_contributions, r.passing = int(cout.n_windows), int(cout.n_contributions), int(cout.passing)
    r.stage_ms = {"build_ms": float(cout.build_ms), "ms1_ms": float(cout.ms1_ms), "trace_ms": float(cout.trace_ms),
                  "integrate_ms": float(cout.integrate_ms), "device_ms": float(cout.device_ms)}
    return r


def lfq_im(features, order, aligned_rt, peptide_q, alignments, ms1, carbon, sulfur, settings, precursor_charge, device: int = 0,
           debug: bool = False) -> LfqResult:
    """lfq for ion-mobility MS1 spectra (sage_hip_lfq_im; lfq.rs:111-127, 267-286, 677-686): every window carries
    Tolerance::Pct(-t, t).bounds(feature.ims), t = settings.mobility_pct_tolerance, and a spectrum whose RawBatch has a mobility
    column keeps a (peak, window) match only if the peak's mobility lies inside.  Spectra without the column are traced as by
    lfq; with no mobility column anywhere the result is lfq's, bit for bit."""
    return lfq(features, order, aligned_rt, peptide_q, alignments, ms1, carbon, sulfur, settings, precursor_charge, device, debug,
               ion_mobility=True)


@dataclass
class ProteinLfqResult:
    """Outputs of sage_hip_protein_lfq, one row per protein id.  log_abundance (natural log, NaN = not quantified),
    intensity (0.0 = not quantified) and component (0xFFFFFFFF = not quantified): [n_proteins, n_files]; pair_median / pair_count
    (debug=True, else None): [n_proteins, n_files (n_files - 1) / 2], (j, k) in lexicographic order."""
    log_abundance: np.ndarray
    intensity: np.ndarray
    component: np.ndarray
    n_rows_used: np.ndarray
    n_components: np.ndarray
    pair_median: Optional[np.ndarray]
    pair_count: Optional[np.ndarray]
    n_batches: int
    stage_ms: dict

    def to_c(self, keep: list) -> "L.SageProteinLfqOutput":
        arr = lambda a, t: (keep.append(a), L.as_ptr(a, t))[1]
        return L.SageProteinLfqOutput(arr(self.log_abundance, C.c_double), arr(self.intensity, C.c_double),
                                      arr(self.component, C.c_uint32), arr(self.n_rows_used, C.c_uint32),
                                      arr(self.n_components, C.c_uint32),
                                      None if self.pair_median is None else arr(self.pair_median, C.c_double),
                                      None if self.pair_count is None else arr(self.pair_count, C.c_uint32))


def protein_lfq(areas, protein_of_row, n_proteins: int, min_ratio_count: int = 1, device: int = 0,
                debug: bool = False) -> ProteinLfqResult:
    """MaxLFQ over precursor rows (sage_hip_protein_lfq).  areas: [n_rows, n_files] f64 (a value that is not a
    positive finite number is missing); protein_of_row: [n_rows] dense ids below n_proteins, 0xFFFFFFFF = the row is ignored.
    debug: also the tables of pair medians and shared-row counts."""
    a = np.ascontiguousarray(areas, dtype=np.float64)
    assert a.ndim == 2
    n_rows, n_files = a.shape
    por = np.ascontiguousarray(protein_of_row, dtype=np.uint32).reshape(-1)
    assert len(por) == n_rows
    n_proteins = int(n_proteins)
    pairs = n_files * (n_files - 1) // 2
    r = ProteinLfqResult(np.full((n_proteins, n_files), np.nan), np.zeros((n_proteins, n_files)),
                         np.full((n_proteins, n_files), 0xFFFFFFFF, np.uint32), np.zeros(n_proteins, np.uint32),
                         np.zeros(n_proteins, np.uint32), np.full((n_proteins, pairs), np.nan) if debug else None,
                         np.zeros((n_proteins, pairs), np.uint32) if debug else None, 0, {})
    cin = L.SageProteinLfqInput(n_rows, n_files, n_proteins, int(min_ratio_count), L.as_ptr(a, C.c_double), L.as_ptr(por, C.c_uint32))
    keep = []
    cout = r.to_c(keep)
    L.check(L.load().sage_hip_protein_lfq(device, C.byref(cin), C.byref(cout)))
    r.n_batches = int(cout.n_batches)
    r.stage_ms = {"log_ms": float(cout.log_ms), "median_ms": float(cout.median_ms), "solve_ms": float(cout.solve_ms),
                  "device_ms": float(cout.device_ms)}
    return r


# ---- roll-up of TMT reporter intensities to proteins / peptides (sage_hip_tmt_rollup) -------------------------------------------
TMT_NORMALISE = {"None": 0, "Total": 1}
TMT_SUMMARY = {"Sum": 0, "Median": 1}


@dataclass
class TmtRollupResult:
    """Outputs of sage_hip_tmt_rollup.  abundance (0.0 = not quantified), log_abundance (natural log, NaN = not
    quantified) and n_cells: [n_groups, n_labels]; n_rows_used: [n_groups]; factor and column_sum: [n_labels].  n_long_groups: the
    groups whose medians were selected over global memory; n_label_slabs: the slabs of 64 channels a wavefront walks per group."""
    abundance: np.ndarray
    log_abundance: np.ndarray
    n_cells: np.ndarray
    n_rows_used: np.ndarray
    factor: np.ndarray
    column_sum: np.ndarray
    n_used_rows: int
    n_long_groups: int
    n_label_slabs: int
    stage_ms: dict


def tmt_rollup(intensity, group_of_row, n_groups: int, min_present: int = 1, normalise: str = "Total", summary: str = "Sum",
               device: int = 0) -> TmtRollupResult:
    """One plex of reporter intensities rolled up to groups (sage_hip_tmt_rollup).  intensity: [n_rows, n_labels] f32,
    as TmtResult.intensity (a cell that is not a positive finite number is missing); group_of_row: [n_rows] ids below n_groups,
    0xFFFFFFFF = the row is ignored; a row counts with at least max(min_present, 1) present cells.  normalise: "Total" | "None";
    summary: "Sum" | "Median"."""
    if normalise not in TMT_NORMALISE:
        raise ValueError(f"normalise: unknown variant `{normalise}`, expected one of " + ", ".join(f"`{v}`" for v in TMT_NORMALISE))
    if summary not in TMT_SUMMARY:
        raise ValueError(f"summary: unknown variant `{summary}`, expected one of " + ", ".join(f"`{v}`" for v in TMT_SUMMARY))
    x = np.ascontiguousarray(intensity, dtype=np.float32)
    assert x.ndim == 2
    n_rows, n_labels = x.shape
    gor = np.ascontiguousarray(group_of_row, dtype=np.uint32).reshape(-1)
    assert len(gor) == n_rows
    n_groups = int(n_groups)
    r = TmtRollupResult(np.zeros((n_groups, n_labels)), np.full((n_groups, n_labels), np.nan), np.zeros((n_groups, n_labels), np.uint32),
                        np.zeros(n_groups, np.uint32), np.ones(n_labels), np.zeros(n_labels), 0, 0, 0, {})
    cin = L.SageTmtRollupInput(n_rows, n_labels, n_groups, int(min_present), TMT_NORMALISE[normalise], TMT_SUMMARY[summary],
                               L.as_ptr(x, C.c_float), L.as_ptr(gor, C.c_uint32))
    cout = L.SageTmtRollupOutput(L.as_ptr(r.abundance, C.c_double), L.as_ptr(r.log_abundance, C.c_double), L.as_ptr(r.n_cells, C.c_uint32),
                                 L.as_ptr(r.n_rows_used, C.c_uint32), L.as_ptr(r.factor, C.c_double), L.as_ptr(r.column_sum, C.c_double))
    L.check(L.load().sage_hip_tmt_rollup(device, C.byref(cin), C.byref(cout)))
    r.n_used_rows, r.n_long_groups, r.n_label_slabs = int(cout.n_used_rows), int(cout.n_long_groups), int(cout.n_label_slabs)
    r.stage_ms = {"norm_ms": float(cout.norm_ms), "summary_ms": float(cout.summary_ms), "device_ms": float(cout.device_ms)}
    return r


# ---- precursor purity of reported PSMs from MS1 scans (sage_hip_precursor_purity) ------------------------------------------------
NO_MS1 = 0xFFFFFFFFFFFFFFFF  # ms1_index of a query without an MS1 spectrum


@dataclass
class PurityResult:
    """Outputs of sage_hip_precursor_purity, one entry per query: peaks in the isolation window and those of them on
    the precursor's isotope envelope, the f64 sums of their intensities and of the peaks one neutron below the precursor, and
    purity = f32(matched / total) (-1.0: no peak in the window, or no MS1 spectrum).  n_sorted_spectra / n_scanned_spectra: the
    spectra with at least one query, by the route they took."""
    n_window: np.ndarray
    n_matched: np.ndarray
    total: np.ndarray
    matched: np.ndarray
    below: np.ndarray
    purity: np.ndarray
    n_sorted_spectra: int
    n_scanned_spectra: int
    stage_ms: dict

    def to_c(self, keep: list) -> "L.SagePurityOutput":
        arr = lambda a, t: (keep.append(a), L.as_ptr(a, t))[1]
        return L.SagePurityOutput(arr(self.n_window, C.c_uint32), arr(self.n_matched, C.c_uint32), arr(self.total, C.c_double),
                                  arr(self.matched, C.c_double), arr(self.below, C.c_double), arr(self.purity, C.c_float))


def precursor_purity(ms1: Sequence[RawBatch], ms1_index, precursor_mz, charge, isolation_lo=None, isolation_hi=None,
                     ppm_tolerance: float = 10.0, max_isotope: int = 4, default_isolation: Tuple[float, float] = (-0.5, 0.5),
                     device: int = 0) -> PurityResult:
    """Precursor purity of one query per entry.  ms1_index: the query's MS1 spectrum, counted through `ms1` in
    order, NO_MS1 for none (assign_ms1 picks them); charge 0 = unknown; isolation offsets in Da, NaN (or no arrays) = the default
    pair, which follows the reference's own fallback (tmt.rs:95-97)."""
    idx = np.ascontiguousarray(ms1_index, dtype=np.uint64).reshape(-1)
    n = len(idx)
    mz = np.ascontiguousarray(precursor_mz, dtype=np.float32).reshape(-1)
    z = np.ascontiguousarray(charge, dtype=np.uint8).reshape(-1)
    assert len(mz) == n and len(z) == n
    lo = hi = None
    if isolation_lo is not None and isolation_hi is not None:
        lo = np.ascontiguousarray(isolation_lo, dtype=np.float32).reshape(-1)
        hi = np.ascontiguousarray(isolation_hi, dtype=np.float32).reshape(-1)
        assert len(lo) == n and len(hi) == n
    r = PurityResult(np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n), np.zeros(n), np.zeros(n), np.full(n, -1.0, np.float32),
                     0, 0, {})
    cb = [b.to_c() for b in ms1]
    arr = (L.SageRawBatch * max(len(cb), 1))(*cb)
    cin = L.SagePurityInput(len(cb), arr, n, L.as_ptr(idx, C.c_uint64), L.as_ptr(mz, C.c_float), L.as_ptr(z, C.c_uint8),
                            None if lo is None else L.as_ptr(lo, C.c_float), None if hi is None else L.as_ptr(hi, C.c_float),
                            L.SagePuritySettings(float(ppm_tolerance), float(default_isolation[0]), float(default_isolation[1]),
                                                 int(max_isotope)))
    keep = []
    cout = r.to_c(keep)
    L.check(L.load().sage_hip_precursor_purity(device, C.byref(cin), C.byref(cout)))
    r.n_sorted_spectra, r.n_scanned_spectra = int(cout.n_sorted_spectra), int(cout.n_scanned_spectra)
    r.stage_ms = {"upload_ms": float(cout.upload_ms), "kernel_ms": float(cout.kernel_ms), "device_ms": float(cout.device_ms)}
    return r


def assign_ms1(ms1: Sequence[RawBatch], file_id, scan_start_time) -> np.ndarray:
    """The MS1 spectrum of each query (file_id, scan_start_time of its MS2 scan), numbered through `ms1` in order: of the spectra of
    the same file_id, the one with the greatest scan_start_time <= t, the later one in the given order among equal times; NO_MS1
    where there is none (a file read as MGF has no MS1).  Host-side numpy."""
    fid = np.asarray(file_id, dtype=np.uint32).reshape(-1)
    t = np.asarray(scan_start_time, dtype=np.float32).reshape(-1)
    assert len(fid) == len(t)
    out = np.full(len(fid), NO_MS1, np.uint64)
    if not len(fid) or not len(ms1):
        return out
    s_fid = np.concatenate([np.asarray(b.file_id, np.uint32) for b in ms1])
    s_t = np.concatenate([np.asarray(b.scan_start_time, np.float32) for b in ms1])
    for f in np.unique(fid):
        spectra = np.flatnonzero((s_fid == f) & ~np.isnan(s_t))
        mine = np.flatnonzero(fid == f)
        if not len(spectra) or not len(mine):
            continue
        by_time = spectra[np.argsort(s_t[spectra], kind="stable")]  # equal times keep the given order: the last one is the later
        k = np.searchsorted(s_t[by_time], t[mine], side="right")     # spectra with time <= t (a NaN t sorts last: guarded below)
        ok = (k > 0) & ~np.isnan(t[mine])
        out[mine[ok]] = by_time[k[ok] - 1].astype(np.uint64)
    return out


# ---- TMT reporter-ion quantification (sage_hip_tmt) ----------------------------------------------------------------------------
# tmt.rs:216-231, as f32
TMT6PLEX = np.array([126.127726, 127.124761, 128.134436, 129.131471, 130.141145, 131.138180], dtype=np.float32)
TMT11PLEX = np.array([126.127726, 127.124761, 127.131081, 128.128116, 128.134436, 129.131471, 129.137790, 130.134825,
                      130.141145, 131.138180, 131.144499], dtype=np.float32)
TMT18PLEX = np.array([126.127726, 127.124761, 127.131081, 128.128116, 128.134436, 129.131471, 129.137790, 130.134825,
                      130.141145, 131.138180, 131.144500, 132.141535, 132.147855, 133.144890, 133.151210, 134.148245,
                      134.154565, 135.15160], dtype=np.float32)
ISOBARIC_VARIANTS = ("Tmt6", "Tmt10", "Tmt11", "Tmt16", "Tmt18", "User")


@dataclass(frozen=True)
class Isobaric:  # tmt.rs:13-61
    kind: str                 # one of ISOBARIC_VARIANTS
    user: Tuple[float, ...] = ()

    def __post_init__(self):
        if self.kind not in ISOBARIC_VARIANTS:
            raise ValueError(f"unknown variant `{self.kind}`, expected one of " + ", ".join(f"`{v}`" for v in ISOBARIC_VARIANTS))

    @staticmethod
    def from_json(obj) -> "Isobaric":
        """serde's externally tagged enum: "Tmt16" or {"User": [f32, ...]}."""
        if isinstance(obj, str) and obj != "User":
            return Isobaric(obj)
        if isinstance(obj, dict) and len(obj) == 1:
            (k, v), = obj.items()
            if k == "User":
                return Isobaric("User", tuple(float(np.float32(x)) for x in v))
            return Isobaric(k)  # (raises, naming the variant)
        raise ValueError(f"unknown variant `{json_text(obj)}`, expected one of " + ", ".join(f"`{v}`" for v in ISOBARIC_VARIANTS))

    def reporter_masses(self) -> np.ndarray:
        return {"Tmt6": TMT6PLEX, "Tmt10": TMT11PLEX[:10], "Tmt11": TMT11PLEX, "Tmt16": TMT18PLEX[:16], "Tmt18": TMT18PLEX,
                "User": np.array(self.user, dtype=np.float32)}[self.kind].copy()

    def modification_mass(self) -> Optional[float]:
        return {"Tmt6": 229.162932, "Tmt10": 229.162932, "Tmt11": 229.162932, "Tmt16": 304.2071, "Tmt18": 304.2135,
                "User": None}[self.kind]

    def headers(self) -> List[str]:
        stem = "user" if self.kind == "User" else "tmt"
        return [f"{stem}_{i + 1}" for i in range(len(self.reporter_masses()))]

    def min_deisotope_mz(self) -> float:
        """runner.rs:398-403 at level 2: reporter_masses().last() * (1.0 + 20E-6) in f32 (last, not max); 0.0 without labels"""
        m = self.reporter_masses()
        return float(m[-1] * (np.float32(1.0) + np.float32(20e-6))) if len(m) else 0.0


def json_text(obj) -> str:
    import json
    return obj if isinstance(obj, str) else json.dumps(obj)


@dataclass
class TmtSettings:  # input.rs:136-160 (TmtSettings::default)
    level: int = 3
    sn: bool = False


@dataclass
class TmtResult:
    """intensity / peak_index: [n_spectra, n_labels], spectra in the order of the batches; peak_index -1 == None."""
    intensity: np.ndarray
    peak_index: np.ndarray
    stage_ms: dict


def tmt(batches: Sequence[RawBatch], isobaric, level: int, take_top_n: int = 150, deisotope: bool = True,
        min_deisotope_mz: float = 0.0, tolerance: Optional[Tolerance] = None, device: int = 0) -> TmtResult:
    """tmt::quantify's reporter intensities (tmt.rs:314-352) on the device for the spectra of `batches` (the spectra of MS level
    `level`; at level 2 they are first processed with SpectrumProcessor(take_top_n, deisotope, min_deisotope_mz), min_peaks 0).
    isobaric: an Isobaric or the label m/z themselves.  tolerance: default Ppm(-20, 20), as the CLI (runner.rs:350)."""
    labels = np.ascontiguousarray(isobaric.reporter_masses() if isinstance(isobaric, Isobaric) else isobaric, dtype=np.float32)
    tol = tolerance or Tolerance("ppm", -20.0, 20.0)
    n = sum(b.n for b in batches)
    nl = len(labels)
    r = TmtResult(np.zeros((n, nl), np.float32), np.full((n, nl), -1, np.int32), {})
    cb = [b.to_c() for b in batches]
    arr = (L.SageRawBatch * max(len(cb), 1))(*cb)
    cin = L.SageTmtInput(len(cb), arr, int(level), nl, L.as_ptr(labels, C.c_float), tol.to_c(), int(take_top_n), int(bool(deisotope)),
                         float(min_deisotope_mz))
    cout = L.SageTmtOutput(L.as_ptr(r.intensity, C.c_float), L.as_ptr(r.peak_index, C.c_int32))
    L.check(L.load().sage_hip_tmt(device, C.byref(cin), C.byref(cout)))
    r.stage_ms = {"upload_ms": float(cout.upload_ms), "process_ms": float(cout.process_ms), "extract_ms": float(cout.extract_ms),
                  "device_ms": float(cout.device_ms)}
    return r
