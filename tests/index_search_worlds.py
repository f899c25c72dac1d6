"""Search worlds over the hand-built index cases (tests/index_cases.py), and one more — `signs_wide_by`, the sign cases among 100
ordinary peptides, so that the large-window kernels meet windows below zero too — TEST INFRASTRUCTURE, CPU only.

tests/test_gpu_index_tables.py holds the TABLES of these databases to a restatement; nothing searched them.  world(name) makes
one of them searchable by both references and by the device: the ArrayDb and its IndexReference, the oracle's database over the
same entries (cut into buckets of 64 or 256 in m/z order, each bucket sorted by peptide: the layout of
Parameters::build_from_peptides, so that the oracle's own pages have their seams inside these databases' tie runs), the peptide
list for tests/second_reading.py, two or three ScorerParams, and ONE batch of spectra whose peaks and precursors are AIMED:

* a peak is aimed at a stored entry e for a fragment tolerance and a fragment charge c when the f32 mass m, found by stepping
  ulps, gives Tolerance::bounds(tol, m * c)[side] == e bit for bit — the entry lies exactly on the window's end; its neighbour
  peak has that bound one ulp on the excluding side of e;
* a precursor m/z is aimed the same way at a pep_mono.

census(world) states the world's conditions on the references alone (no device result enters it).  Run as a script, the module
writes every world's census to profiles/index_search_census.json; tests/test_index_search_cpu.py holds the file to a fresh
census."""
import ctypes as C
import json
import os
import sys

import numpy as np

if __name__ == "__main__":  # (as a script: the package lies beside tests/)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oracle_lib
import second_reading as SR
from index_cases import BY, HAND_BUILT, T2, Pep, database, random_peptides
import index_reference
from index_reference import F32, IndexReference, total_order_key
from sage_amd import _lib as L
from sage_amd.api import ScorerParams, SpectrumBatch, Tolerance



def signs_wide():
    """index_cases.signs among 100 ordinary peptides: more than 64 slots in a whole-database window, so that the large-window count
    and replay kernels meet windows below and across zero as well (SAGE_HIP_WCAP cannot go below 64)"""
    rng = np.random.default_rng(77)
    peps = random_peptides(rng, 100, 3, 8)
    for p in random_peptides(rng, 16, 3, 8):
        peps.append(Pep(p.seq, [-500.0] + [0.0] * (len(p.seq) - 1)))                               # leading b-ions below zero
    for p in random_peptides(rng, 8, 3, 8):
        peps.append(Pep(p.seq, [-index_reference.RESIDUE_MASS[p.seq[0]]] + [0.0] * (len(p.seq) - 1)))  # b1 == 0.0 exactly
    for p in random_peptides(rng, 6, 3, 6):
        peps.append(Pep(p.seq, [0.0] * (len(p.seq) - 1) + [-900.0], mono=F32(40.0)))               # y-ions below zero
    return database(peps, BY, 0)


# the hand-built cases, and one more that only the searches need
ALL_CASES = list(HAND_BUILT) + [("signs_wide_by", T2, signs_wide)]
CASES = {name: (env, build) for name, env, build in ALL_CASES}
NAMES = [c[0] for c in ALL_CASES]
CENSUS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "index_search_census.json")
PEAKS = 150          # at most, per spectrum
SECOND_READING_SAMPLE = 8   # spectra of seam_large_4133 the brute-force reading scores
INF = F32(np.inf)


def bits(x):
    return int(np.asarray(x, F32).view(np.uint32))


def key(x):
    return int(total_order_key(np.asarray([x], F32))[0])


def up(x, n=1):
    x = F32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, INF if n > 0 else -INF)
    return x


def tol_tuple(t):
    return (t.kind, t.lo, t.hi)


def fragment_charges(params, z):
    """the fragment charges Scorer::matched_peaks tries for a precursor of charge z (scoring.rs:239-247, 359)"""
    return range(1, SR.max_fragment_charge(params.max_fragment_charge, z))


# ---- aiming --------------------------------------------------------------------------------------------------------------------
def _step_to(f, x, target, steps=48):
    """an f32 x near the given one with f(x) == target bit for bit (f non-decreasing in x), or None"""
    want = key(target)
    x = F32(x)
    with np.errstate(all="ignore"):
        got = key(f(x))
        if got == want:
            return x
        d = 1 if got < want else -1
        for _ in range(steps):
            x = up(x, d)
            got = key(f(x))
            if got == want:
                return x
            if (got < want) != (d > 0):
                return None
    return None


def _centre_for(tol, t, e):
    kind = tol[0]
    if kind == "da":
        return float(e) - float(t)
    return float(e) / (1.0 + float(t) * (1e-6 if kind == "ppm" else 1e-2))


def aim_peak(tol, c, e, side):
    """the mass of a peak whose window for fragment charge c has bounds(tol, m * c)[side] == e"""
    guess = _centre_for(tol, tol[1 + side], e) / c
    return _step_to(lambda m: SR.bounds(tol, F32(m) * F32(c))[side], guess, e)


def precursor_mass(mz, z):
    return (F32(mz) - SR.PROTON) * F32(z)   # scoring.rs:420, 438


def aim_precursor(tol, z, mono, side):
    """a precursor m/z whose window at charge z has bounds(tol, mass)[side] == mono"""
    guess = _centre_for(tol, tol[1 + side], mono) / z + float(SR.PROTON)
    return _step_to(lambda mz: SR.bounds(tol, precursor_mass(mz, z))[side], guess, mono)


def holding_precursor(tol, z, mono):
    """a precursor m/z whose window at charge z holds `mono` well inside (not aimed)"""
    return F32(_centre_for(tol, 0.5 * (float(tol[1]) + float(tol[2])), mono) / z + float(SR.PROTON))


# ---- the oracle's database over a hand-built list -----------------------------------------------------------------------------
class BucketedDb:
    """The oracle's database over a hand-built list: the entries in m/z order (then peptide), cut into buckets, each sorted by
    peptide; min_value is a bucket's first m/z BEFORE that sort (database.rs:321-337)."""

    def __init__(self, db, ref, bucket_size):
        s = ref.sorted_entries().copy()
        self.min_value = s["fragment_mz"][::bucket_size].copy()   # (a copy: the buckets are sorted in place below)
        for a in range(0, len(s), bucket_size):
            chunk = s[a:a + bucket_size]
            s[a:a + bucket_size] = chunk[np.argsort(chunk["peptide_index"], kind="stable")]
        self.fragments, self.bucket_size, self.db = s, bucket_size, db

    def oracle(self):
        """(OracleDb.from_product's call, with a real pointer behind every empty array: it is never read)"""
        lib, db = oracle_lib.load(), self.db
        keep = []

        def ptr(a, t):
            a = np.ascontiguousarray(a)
            keep.append(a if len(a) else np.zeros(1, a.dtype))
            return L.as_ptr(keep[-1], t)
        h = lib.orc_db_from_arrays(ptr(self.fragments["peptide_index"], C.c_uint32), ptr(self.fragments["fragment_mz"], C.c_float),
                                   len(self.fragments), ptr(self.min_value, C.c_float), len(self.min_value), self.bucket_size,
                                   ptr(db.pep_mono, C.c_float), ptr(db.seq_off, C.c_uint64), ptr(db.seq, C.c_uint8), ptr(db.mods, C.c_float),
                                   ptr(db.nterm, C.c_float), ptr(db.cterm, C.c_float), ptr(db.decoy, C.c_uint8),
                                   ptr(db.missed_cleavages, C.c_uint8), db.n_peptides, ptr(db.ion_kinds, C.c_uint8), len(db.ion_kinds))
        return oracle_lib.OracleDb(C.c_void_p(h))


# ---- settings ------------------------------------------------------------------------------------------------------------------
def settings_of(name, index, db):
    """two or three ScorerParams per world; across the worlds: ppm / Da / Pct fragment tolerances, max_fragment_charge 1 and 2,
    min_matched_peaks 0 and 1, report_psms 1..3, and in every world a Da precursor window that takes in the whole database"""
    mono = db.pep_mono
    span = float(mono[-1] - mono[0]) + 50.0 if len(mono) else 50.0
    whole = Tolerance("da", -span, span)
    if name.startswith(("signs", "cell_edges")):
        return [ScorerParams(precursor_tol=whole, fragment_tol=Tolerance("da", -0.5, 0.5), max_fragment_charge=2, min_matched_peaks=1, report_psms=3),
                ScorerParams(precursor_tol=Tolerance("da", -1.0, 1.0), fragment_tol=Tolerance("da", -0.01, 0.01), max_fragment_charge=1,
                             min_matched_peaks=0, report_psms=1),
                ScorerParams(precursor_tol=whole, fragment_tol=Tolerance("ppm", -10.0, 10.0), max_fragment_charge=2, min_matched_peaks=1, report_psms=2)]
    if index % 2 == 0:
        return [ScorerParams(precursor_tol=whole, fragment_tol=Tolerance("ppm", -10.0, 10.0), max_fragment_charge=2, min_matched_peaks=1, report_psms=3),
                ScorerParams(precursor_tol=Tolerance("ppm", -20.0, 20.0), fragment_tol=Tolerance("pct", -0.002, 0.002), max_fragment_charge=1,
                             min_matched_peaks=0, report_psms=1)]
    return [ScorerParams(precursor_tol=whole, fragment_tol=Tolerance("da", -0.02, 0.01), max_fragment_charge=2, min_matched_peaks=0, report_psms=2),
            ScorerParams(precursor_tol=Tolerance("ppm", 5.0, 50.0), fragment_tol=Tolerance("ppm", -10.0, 10.0), max_fragment_charge=1,
                         min_matched_peaks=1, report_psms=1)]   # (a one-sided precursor window: the centre lies below it)


def geometry(env):
    """(small-tile shift, large-tile shift) of the case's own environment (capi_db.hip's clamps)"""
    return min(16, max(6, int(env.get("SAGE_HIP_TILE2_SHIFT", 11)))), min(15, max(11, int(env.get("SAGE_HIP_TILE_SHIFT", 15))))


# ---- the world -----------------------------------------------------------------------------------------------------------------
class SearchWorld:
    pass


_worlds = {}


def world(name):
    if name not in _worlds:
        _worlds[name] = _build(name)
    return _worlds[name]


def _aimed_entries(name, db, ref, env):
    """[(what, m/z)]: the stored m/z the world's peaks are aimed at"""
    out = []
    if ref.nf == 0:
        return out, {}
    for label, shift in zip(("small", "large"), geometry(env)):
        copy, toff = ref.tile_copy(shift)["fragment_mz"], ref.tile_offsets(shift)
        for t in range(len(toff) - 1):
            if toff[t + 1] > toff[t]:
                out += [(f"{label} tile {t} first", copy[toff[t]]), (f"{label} tile {t} last", copy[toff[t + 1] - 1])]
    mz, pep = ref.entries["fragment_mz"], ref.entries["peptide_index"]
    s = ref.sorted_entries()["fragment_mz"]
    if name.startswith("cell_edges"):
        out += [("edge entry", m) for m in s]                      # every entry is an edge or an edge's neighbour (index_cases.cell_edges)
        out += [("top", s[-1])]
    if name.startswith("signs"):
        neg = s[s < 0]
        out += [("zero", F32(0.0))] + [("negative", m) for m in list(neg[:3]) + list(neg[-3:])]
    if name == "ties":
        out += [("tie run", m) for m in mz[pep == 61][:4]]         # peptides 59..65 share every entry
        first = mz[pep == 0]
        dup = [m for m in first if (first.view(np.uint32) == bits(m)).sum() == 2][0]
        out += [("GGG double", dup)]
    if name == "empty_middle":
        # the nearest ends of the two tiles that hold entries: the light tile's last m/z and the heavy tile's first (small tiles 0
        # and 2 at shift 6); tile 1 between them holds nothing
        copy, toff = ref.tile_copy(6)["fragment_mz"], ref.tile_offsets(6)
        assert toff[1] == toff[2] and copy[toff[1] - 1] < copy[toff[2]], "the light tile ends below the heavy tile's start"
        out += [("light tile's end", copy[toff[1] - 1]), ("heavy tile's start", copy[toff[2]])]
    seen, uniq, special = set(), [], {}
    for what, m in out:  # (an m/z aimed at for two reasons keeps its first label in the list; `special` knows every reason)
        special.setdefault(what, set()).add(bits(m))
        if bits(m) not in seen:
            seen.add(bits(m))
            uniq.append((what, F32(m)))
    return uniq, special


def _build(name):
    env, build = CASES[name]
    index = NAMES.index(name)
    rng = np.random.default_rng([2027, index])
    w = SearchWorld()
    w.name, w.env, w.index = name, env, index
    w.db = db = build()
    w.ref = ref = IndexReference(db)
    w.bucket_size = 64 if index % 2 == 0 or name == "ties" else 256
    w.bucketed = BucketedDb(db, ref, w.bucket_size)
    w.settings = settings_of(name, index, db)
    w.kinds, w.min_ion_index = [int(k) for k in db.ion_kinds], db.min_ion_index
    ftols, ptols = [], []
    for p in w.settings:
        if tol_tuple(p.fragment_tol) not in ftols:
            ftols.append(tol_tuple(p.fragment_tol))
        if tol_tuple(p.precursor_tol) not in ptols:
            ptols.append(tol_tuple(p.precursor_tol))
    narrow = ptols[1]
    mono, n = db.pep_mono, db.n_peptides
    w.aimed, w.special = _aimed_entries(name, db, ref, env)
    w.aims = []       # (spectrum, entry bits, tolerance, charge, side, "exact" / "neighbour", mass)
    w.precursor_aims = []  # (spectrum, what, peptide, tolerance, charge, side)
    plans = []        # (precursor m/z, charge, [peak masses])
    has = np.diff(ref.pm_off.astype(np.int64)) > 0 if n else np.zeros(0, bool)

    def own_peaks(spec, p, limit=5):
        """exact peaks at a few of peptide p's own stored entries, for every fragment tolerance: the spectrum reports p"""
        masses = []
        if p is None or not has.any():
            return masses
        if not has[p]:  # no stored entry of its own: peaks at the nearest peptides that have some, below and above — real fragment
            # windows in front of a precursor window that may hold no entry at all
            below, above = np.flatnonzero(has[:p]), p + 1 + np.flatnonzero(has[p + 1:])
            for q in ([int(below[-1])] if len(below) else []) + ([int(above[0])] if len(above) else []):
                masses += own_peaks(spec, q, limit)
            return masses
        mz = ref.entries["fragment_mz"][int(ref.pm_off[p]):int(ref.pm_off[p + 1])]
        for e in mz[np.linspace(0, len(mz) - 1, min(limit, len(mz))).astype(int)]:
            for tol in ftols:
                m = aim_peak(tol, 1, e, int(rng.integers(0, 2)))
                if m is not None:
                    masses.append(m)
                    w.aims.append((spec, bits(e), tol, 1, None, "own", m))
        return masses

    def precursor(spec, what, p, side, tol=narrow):
        for z in (3, 2):
            mz = aim_precursor(tol, z, mono[p], side)
            if mz is not None:
                w.precursor_aims.append((spec, what, p, tol, z, side))
                return mz, z
        return holding_precursor(tol, 3, mono[p]), 3   # (not landed: the window still holds p)

    if n == 0:   # `empty`: nothing to aim at — three ordinary spectra
        for i in range(3):
            plans.append((F32(400.0 + 10.0 * i), 2, list(np.sort(rng.uniform(100.0, 900.0, 40)).astype(F32))))
    else:
        homes = [(0, 0, "first peptide"), (0, 1, "first peptide"), (n - 1, 0, "last peptide"), (n - 1, 1, "last peptide")]
        if name == "ties":
            homes += [(9, 0, "tie run 9..12"), (12, 1, "tie run 9..12"), (59, 0, "tie run 59..65"), (65, 1, "tie run 59..65")]
        if name == "empty_middle":
            homes += [(64, 0, "only the tile without entries"), (127, 1, "only the tile without entries"), (96, 0, "only the tile without entries")]
        for p, side, what in homes:
            mz, z = precursor(len(plans), what, p, side)
            plans.append((mz, z, own_peaks(len(plans), p)))
        # a mass below and above every peptide (the narrow windows select nothing)
        stored = np.flatnonzero(has)
        for what, mass, p in (("below every peptide", float(mono[0]) - 7.0, stored[0] if len(stored) else None),
                              ("above every peptide", float(mono[-1]) + 7.0, stored[-1] if len(stored) else None)):
            w.precursor_aims.append((len(plans), what, None, narrow, 3, None))
            plans.append((F32(mass / 3.0 + float(SR.PROTON)), 3, own_peaks(len(plans), p)))
        # the aimed entries: exact and neighbour peaks, charges 1 and 2, both sides, every fragment tolerance of the world
        peaks = []
        for what, e in w.aimed:
            for tol in ftols:
                for c in (1, 2):
                    for side in (0, 1):
                        m = aim_peak(tol, c, e, side)
                        if m is not None:
                            peaks.append((bits(e), tol, c, side, "exact", m))
                        m = aim_peak(tol, c, up(e, 1 if side == 0 else -1), side)
                        if m is not None:
                            peaks.append((bits(e), tol, c, side, "neighbour", m))
        extra = []
        if name.startswith("cell_edges"):   # a window that lies wholly above the table's top entry
            extra.append(F32(float(ref.sorted_entries()["fragment_mz"][-1]) * 1.01 + 1.5))
        if name.startswith("signs"):        # Da +-0.5 around 0.25: from cell 0's negative run into the first positive cells
            extra.append(F32(0.25))
        if name == "empty_middle":          # windows in the gap between the light tile's end and the heavy tile's start
            a, b = [float(np.array([next(iter(w.special[k]))], np.uint32).view(F32)[0]) for k in ("light tile's end", "heavy tile's start")]
            extra += [F32(0.5 * (a + b)), F32(0.5 * (a + b) / 2.0)]
        home = int(stored[len(stored) // 2]) if len(stored) else n // 2
        room = PEAKS - 5 * len(ftols) - len(extra) - 2
        for a in range(0, max(len(peaks), 1), room):
            spec = len(plans)
            mz, z = precursor(spec, "a peptide in the middle", home, 0)
            if z != 3:   # (charge-2 fragments need a precursor charge of 3: scoring.rs:239-247)
                mz, z = holding_precursor(narrow, 3, mono[home]), 3
                w.precursor_aims.pop()
            chunk = peaks[a:a + room]
            w.aims += [(spec,) + pk for pk in chunk]
            plans.append((mz, z, own_peaks(spec, home) + [pk[-1] for pk in chunk] + extra))
        ordinary = 0
        while ordinary < 3 or len(plans) < 8:  # ordinary spectra of peptides drawn from the list (those with entries, if any)
            p = int(rng.choice(stored)) if len(stored) else int(rng.integers(0, n))
            plans.append((holding_precursor(narrow, 2, mono[p]), 2, own_peaks(len(plans), p, 12)))
            ordinary += 1
    # the batch: masses ascending in the total order, no mass twice, seeded intensities, the TIC summed in f32 in peak order
    off, masses, intens, tic = [0], [], [], []
    for mz, z, pk in plans:
        m = np.array(pk, F32)
        m = m[np.isfinite(m)] if len(m) else m
        m = m[np.argsort(total_order_key(m), kind="stable")] if len(m) else m
        if len(m):
            m = m[np.concatenate([[True], m[1:].view(np.uint32) != m[:-1].view(np.uint32)])]
        assert len(m) <= PEAKS, (name, len(m))
        it = (rng.integers(1, 9, len(m)) * 250).astype(F32)
        off.append(off[-1] + len(m))
        masses.append(m)
        intens.append(it)
        tic.append(np.cumsum(it, dtype=F32)[-1] if len(it) else F32(0.0))
    cat = lambda xs: np.concatenate(xs).astype(F32) if xs else np.zeros(0, F32)
    k = len(plans)
    w.batch = SpectrumBatch(np.array(off, np.uint64), cat(masses), cat(intens), [p[0] for p in plans], [p[1] for p in plans], tic,
                            None, None, np.arange(k, dtype=F32) * F32(0.5), None, np.zeros(k, np.uint32))
    w.second_reading_spectra = np.arange(k)
    if name == "seam_large_4133":
        w.second_reading_spectra = np.sort(rng.choice(k, min(k, SECOND_READING_SAMPLE), replace=False))
    w.oracle = w.bucketed.oracle()
    w.with_fragments = db.with_fragments(ref.sorted_entries())   # the host route of a device database: the stored entries by m/z
    return w


def peptide_arrays(w):
    """what second_reading.Peptides takes, from the ArrayDb alone"""
    db = w.db
    return dict(pep_mono=db.pep_mono, seq_off=db.seq_off, seq=db.seq, mods=db.mods, nterm=db.nterm, decoy=db.decoy, missed=db.missed_cleavages)


# ---- the census ----------------------------------------------------------------------------------------------------------------
def census(w):
    """The world's conditions, asserted on the references alone.  Returns the figures."""
    name, b, ref, db = w.name, w.batch, w.ref, w.db
    out = dict(world=name, bucket_size=w.bucket_size, peptides=db.n_peptides, entries=ref.nf, spectra=b.n,
               peaks=int(b.peak_off[-1]), aimed_entries=len(w.aimed))
    assert 2 <= len(w.settings) <= 3
    assert (np.diff(b.peak_off.astype(np.int64)) <= PEAKS).all()
    for i in range(b.n):
        m = b.masses[int(b.peak_off[i]):int(b.peak_off[i + 1])]
        assert (np.diff(total_order_key(m)) > 0).all(), "masses ascending in the total order"
    entry_bits = set(ref.entries["fragment_mz"].view(np.uint32).tolist())
    mono_bits = set(db.pep_mono.view(np.uint32).tolist())
    s_mz = ref.sorted_entries()["fragment_mz"]
    # every aimed peak does what it was aimed to do
    hit = set()
    for spec, eb, tol, c, side, how, m in w.aims:
        a, z = int(b.peak_off[spec]), int(b.peak_off[spec + 1])
        assert bits(m) in set(b.masses[a:z].view(np.uint32).tolist()), (name, "an aimed peak is in its spectrum")
        if how == "own":
            continue
        bound = SR.bounds(tol, F32(m) * F32(c))[side]
        e = np.array([eb], np.uint32).view(F32)[0]
        if how == "exact":
            assert bits(bound) == eb, (name, how, tol, c, side)
            hit.add(eb)
        else:
            assert bits(bound) == bits(up(e, 1 if side == 0 else -1)), (name, how, tol, c, side)
    out["aimed_entries_hit_exactly"] = len(hit)
    # the windows the searches really open: per setting, spectrum, peak and fragment charge
    ends = straddles = below_zero = wide32 = wide256 = above_top = zero_end = negative_end = spans_zero = 0
    tie_lo = tie_hi = ggg = edge_end = top_end = light_end = heavy_start = in_gap = 0
    tie_bits, dup_bits = w.special.get("tie run", set()), w.special.get("GGG double", set())
    edge_bits = w.special.get("edge entry", set()) | w.special.get("top", set())
    light_bits, heavy_bits = w.special.get("light tile's end", set()), w.special.get("heavy tile's start", set())
    gap = [np.array([next(iter(x))], np.uint32).view(F32)[0] for x in (light_bits, heavy_bits)] if light_bits else None
    prec_ends, prec_windows, empty_tile_only = 0, 0, 0
    psm_spectra = {}
    for k, p in enumerate(w.settings):
        ftol, ptol = tol_tuple(p.fragment_tol), tol_tuple(p.precursor_tol)
        feats, counts, _, _ = w.oracle.score(p, b)
        psm_spectra[k] = int((counts > 0).sum())
        for i in range(b.n):
            z = int(b.precursor_charge[i])
            plo, phi = SR.bounds(ptol, precursor_mass(b.precursor_mz[i], z))
            prec_windows += 1
            prec_ends += bits(plo) in mono_bits or bits(phi) in mono_bits
            if name == "empty_middle" and db.n_peptides:
                sel = np.flatnonzero((db.pep_mono >= plo) & (db.pep_mono <= phi))
                if len(sel) and sel[0] >= 64 and sel[-1] <= 127:
                    empty_tile_only += 1
                    assert counts[i] == 0, "peptides without a stored entry give no candidate"
                    assert b.peak_off[i + 1] - b.peak_off[i] >= 4, "... in front of real fragment windows"
            for m in b.masses[int(b.peak_off[i]):int(b.peak_off[i + 1])]:
                for c in fragment_charges(p, z):
                    lo, hi = SR.bounds(ftol, F32(m) * F32(c))
                    bl, bh = bits(lo), bits(hi)
                    ends += bl in entry_bits or bh in entry_bits
                    with np.errstate(all="ignore"):
                        straddles += np.floor(float(lo) * 32.0) != np.floor(float(hi) * 32.0)
                        wide32 += (float(hi) - float(lo)) * 32.0 >= 16.0
                        wide256 += (float(hi) - float(lo)) * 256.0 >= 128.0
                    below_zero += lo < 0
                    spans_zero += lo < 0 < hi
                    above_top += ref.nf > 0 and lo > s_mz[-1]
                    zero_end += (bl == 0 or bh == 0) and 0 in entry_bits
                    negative_end += (lo < 0 and bl in entry_bits) or (hi < 0 and bh in entry_bits)
                    tie_lo += bl in tie_bits
                    tie_hi += bh in tie_bits
                    ggg += bl in dup_bits or bh in dup_bits
                    edge_end += bl in edge_bits or bh in edge_bits
                    top_end += ref.nf > 0 and (bl == bits(s_mz[-1]) or bh == bits(s_mz[-1]))
                    light_end += bl in light_bits or bh in light_bits
                    heavy_start += bl in heavy_bits or bh in heavy_bits
                    in_gap += gap is not None and gap[0] < lo <= hi < gap[1]
    out.update(fragment_windows_ending_on_an_entry=int(ends), fragment_windows_straddling_a_cell_edge=int(straddles),
               fragment_windows_starting_below_zero=int(below_zero), precursor_windows=prec_windows,
               precursor_windows_ending_on_a_pep_mono=int(prec_ends), spectra_with_a_psm=[psm_spectra[k] for k in sorted(psm_spectra)])
    # ---- conditions, not measurements
    assert sorted({p.max_fragment_charge for p in w.settings}) == [1, 2] and {p.min_matched_peaks for p in w.settings} == {0, 1}
    assert db.n_peptides == 0 or any(p.precursor_tol.kind == "da" and -p.precursor_tol.lo > float(db.pep_mono[-1] - db.pep_mono[0]) for p in w.settings)
    if db.n_peptides == 0:
        assert b.n == 3 and all(v == 0 for v in psm_spectra.values())
        return out
    assert 8 <= b.n <= 24, (name, b.n)
    if ref.nf:
        assert 3 * len(hit) >= 2 * len(w.aimed), f"{name}: {len(hit)} of {len(w.aimed)} aimed entries hit exactly"
        assert ends > 0 and straddles > 0
        assert all(3 * v >= b.n for v in psm_spectra.values()), f"{name}: spectra with a PSM per setting {psm_spectra} of {b.n}"
    whats = {a[1] for a in w.precursor_aims}
    assert {"below every peptide", "above every peptide"} <= whats
    landed = {(a[1], a[5]) for a in w.precursor_aims if a[2] is not None}
    assert prec_ends > 0 and {w_ for w_, _ in landed} >= {"first peptide", "last peptide"}, (name, landed)
    if name.startswith("cell_edges"):
        assert edge_end >= len(edge_bits) and top_end > 0 and above_top > 0
        out.update(windows_ending_on_an_edge_entry=int(edge_end), windows_above_the_top=int(above_top))
    if name.startswith(("signs", "cell_edges")):
        assert wide32 > 0 and wide256 > 0
        out.update(windows_of_16_cells_and_more=int(wide32))
    if name.startswith("signs"):
        assert zero_end > 0 and negative_end > 0 and spans_zero > 0 and below_zero > 0
        out.update(windows_ending_on_zero=int(zero_end), windows_ending_on_a_negative_entry=int(negative_end), windows_across_zero=int(spans_zero))
    if name == "ties":
        assert tie_lo > 0 and tie_hi > 0 and ggg > 0
        assert {("tie run 59..65", 0), ("tie run 59..65", 1), ("tie run 9..12", 0), ("tie run 9..12", 1)} <= landed, landed
        s = ref.sorted_entries()
        same = s["fragment_mz"][1:].view(np.uint32) == s["fragment_mz"][:-1].view(np.uint32)
        seam = np.arange(1, len(s)) % w.bucket_size == 0
        assert (same & seam).any(), "a seam of the oracle's buckets inside a run of equal m/z"
        out.update(windows_starting_on_the_tie_run=int(tie_lo), windows_ending_on_the_tie_run=int(tie_hi), windows_on_the_double_entry=int(ggg),
                   bucket_seams_inside_a_tie_run=int((same & seam).sum()))
    if name == "empty_middle":
        assert empty_tile_only > 0
        # fragment windows on the nearest ends of the light and the heavy tile, and in the gap between them: nothing of tile 1
        assert light_end > 0 and heavy_start > 0 and in_gap > 0
        out.update(precursor_windows_inside_the_empty_tile=int(empty_tile_only), windows_on_the_light_tiles_end=int(light_end),
                   windows_on_the_heavy_tiles_start=int(heavy_start), windows_in_the_gap_between_them=int(in_gap))
    return out


if __name__ == "__main__":
    figures = [census(world(n)) for n in NAMES]
    with open(CENSUS_FILE, "w") as f:
        json.dump(figures, f, indent=1)
        f.write("\n")
    print(f"{len(figures)} worlds -> {CENSUS_FILE}")
