"""The two-kind instance of rescore_kernel (kernels.hip: KINDS2 — a database of exactly two ion kinds, the first n-terminal, the
second not; picked once per scorer, capi.hip: scorer_init) against the general instance (SAGE_HIP_RESCORE_KINDS_GENERAL=1, read when
the scorer is created) and the oracle.  Per database and setting of SAGE_HIP_DEBUG_FLAGS in

    0, 32, 64 | 32768, 64 | 32768 | 262144, 128, 8192, 16384

the records of the two are equal byte for byte and equal to the oracle's, and sage_hip_debug_rescore_instance confirms the instance
each case names:

    takes the two-kind instance    {b, y}, {c, z}, {a, x}
    keeps the general one          {y, b} (kind 0 not n-terminal), {b} alone, {b, y, c}, the six kinds, a chimera search,
                                   SAGE_HIP_RESCORE_GENERAL=1

The spectra are made here, from each database's own ion kinds, at the shapes at which the decode can go wrong: peptides of 33, 34
and 35 residues (64, 66 and 68 ions: the kind boundary at bit 32 of a full chunk; two ions in the second chunk; a second chunk that
starts inside kind 1 at index 30), the longest peptides of the world (more than 65 residues: a whole chunk inside kind 0) and the
shortest the digest allows (2 to 5 residues: one-bit segments; 5 is the first that the fragment index can put on a candidate list);
precursor charges 2, 3, 4 and 5 (one, two, three fragment charges on the filter, four unfiltered); fragment ladders on both sides of
the kind boundary, on the n-terminal side only and on the other side only; and spectra whose peaks lie below every fragment (nothing
matches).  The high-charge world of tests/test_gpu_rescore_heavy_adds.py adds
charges 4 to 6 in C3-like lists.  A few hundred spectra in all.

Not vacuous: under 64 | 32768 the profiling instance (SAGE_HIP_PHASE_CLOCKS=1: PROF | KINDS2) must count chunks and matches on the
cooperative path, one-trip and per-charge routes both."""
import ctypes as C

import numpy as np
import pytest

from parity_utils import assert_features_equal
from sage_amd import _lib as L
from sage_amd.api import RawSpectrum, Scorer, ScorerParams, SpectrumBatch, SpectrumProcessor
from sage_amd.synthetic import _MASS_LUT, PROTON
from test_gpu_rescore_heavy_adds import high_charge_world, length_world  # noqa: F401  (the fixture and the world's recipe)

pytestmark = pytest.mark.gpu

NO_COOP, EVERY_HEAVY, WALK, PER_LANE, FLAT_ALWAYS, FIRST_HIT, PER_CHARGE = 32, 64, 128, 8192, 16384, 32768, 262144
FLAG_SETS = (0, NO_COOP, EVERY_HEAVY | FIRST_HIT, EVERY_HEAVY | FIRST_HIT | PER_CHARGE, WALK, PER_LANE, FLAT_ALWAYS)
ENV = ("SAGE_HIP_RESCORE_GENERAL", "SAGE_HIP_RESCORE_KINDS_GENERAL", "SAGE_HIP_DEBUG_FLAGS", "SAGE_HIP_PHASE_CLOCKS")
INST_CHIMERA, INST_KINDS2, INST_FAST, INST_ACC, INST_PROF, INST_BIG = 1, 2, 4, 8, 16, 32

TWO_KINDS = {"by": ["b", "y"], "cz": ["c", "z"], "ax": ["a", "x"]}
GENERAL = {"yb": ["y", "b"], "b": ["b"], "byc": ["b", "y", "c"], "abcxyz": ["a", "b", "c", "x", "y", "z"]}

# ion_series.rs:36-53 — the series' offsets from the b resp. y series
_C, _O, _H, _N = 12.0, 15.994914, 1.007825, 14.003074
_NH3 = _N + 2.0 * _H + 1.0072764
SERIES = {"a": (0, -(_C + _O)), "b": (0, 0.0), "c": (0, _NH3), "x": (1, _C + _O - _NH3 + _N + _H), "y": (1, 0.0), "z": (1, -_NH3)}


def made_spectra(host, kinds, seed):
    """(batch, what): per peptide length of interest x charge 2 .. 5 x {both sides, n-terminal side only, other side only}, then the
    spectra that match nothing"""
    rng = np.random.default_rng(seed)
    seq_off = host.seq_off.astype(np.int64)
    lens = np.diff(seq_off)
    targets = np.flatnonzero(host.decoy == 0)
    tl = lens[targets]
    longest = int(tl.max())
    assert {2, 5, 33, 34, 35} <= set(tl.tolist()) and longest > 65, sorted(set(tl.tolist()))
    raws, what = [], []
    for plen, take in ((2, 2), (3, 2), (4, 2), (5, 2), (33, 3), (34, 3), (35, 3), (longest, 2)):
        for pep in targets[tl == plen][:take]:
            a, b = seq_off[pep], seq_off[pep + 1]
            res = _MASS_LUT[host.seq[a:b]] + host.mods[a:b].astype(np.float64)
            nterm = float(host.nterm[pep]) if not np.isnan(host.nterm[pep]) else 0.0
            mono = float(host.pep_mono[pep])
            bs = nterm + np.cumsum(res)[:-1]
            ys = mono - bs  # (index order of the table: the longest y ion first)
            n = len(bs)
            for z in (2, 3, 4, 5):
                for sides in ("both", "n", "c"):
                    # a ladder with a gap and a few lone ions per side; the last indices among them (the ions of the last chunk)
                    start = int(rng.integers(0, max(1, n - 8)))
                    idx = np.unique(np.concatenate([np.arange(start, min(n, start + 9)), rng.integers(0, n, 3), [n - 1, max(0, n - 2)]]))
                    idx = idx[idx != start + 4]
                    mzs = []
                    for k in kinds:
                        side, off = SERIES[k]
                        if sides != "both" and (sides == "n") != (side == 0):
                            continue
                        frag = (bs if side == 0 else ys)[idx] + off
                        for c in range(1, min(z - 1, 3) + 1):
                            sel = frag if c == 1 else frag[rng.random(len(frag)) < 0.6]
                            mzs.append((sel + c * PROTON) / c)
                    mz = np.concatenate(mzs + [rng.uniform(100.0, 1500.0, 12)])
                    mz = mz[mz > 50.0] * (1.0 + rng.normal(0.0, 2.0, int((mz > 50.0).sum())) * 1e-6)
                    it = rng.lognormal(8.0, 1.0, len(mz))
                    order = np.argsort(mz, kind="stable")
                    raws.append(RawSpectrum(mz[order].astype(np.float32), it[order].astype(np.float32), float(np.float32((mono + z * PROTON) / z)),
                                            z, None, scan_start_time=float(len(raws)), file_id=0, id=f"scan={len(raws) + 1}"))
                    what.append((plen, z, sides))
            # nothing matches: every peak lighter than any fragment of any series
            mz = np.sort(rng.uniform(20.0, 28.0, 8))
            raws.append(RawSpectrum(mz.astype(np.float32), rng.lognormal(8.0, 1.0, 8).astype(np.float32), float(np.float32((mono + 2 * PROTON) / 2)),
                                    2, None, scan_start_time=float(len(raws)), file_id=0, id=f"scan={len(raws) + 1}"))
            what.append((plen, 2, "none"))
    sp = SpectrumProcessor(150, False, 0.0)
    return SpectrumBatch.from_spectra([sp.process(r) for r in raws]), what


class Case:
    def __init__(self, name, kinds):
        self.world = length_world(kinds)
        self.batch, self.what = made_spectra(self.world.host, kinds, seed=59 + len(name))
        self.oracle = {}

    def expected(self, params):
        key = repr(params)
        if key not in self.oracle:
            self.oracle[key] = self.world.orc.score(params, self.batch)[:2]
        return self.oracle[key]


@pytest.fixture(scope="module")
def cases(gpu_required):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, {**TWO_KINDS, **GENERAL}[name])
        return made[name]
    return get


def run(dev, batch, params, monkeypatch, flags=0, kinds_general=False, general=False, clocks=False):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    if general:
        monkeypatch.setenv("SAGE_HIP_RESCORE_GENERAL", "1")
    if kinds_general:
        monkeypatch.setenv("SAGE_HIP_RESCORE_KINDS_GENERAL", "1")
    if flags:
        monkeypatch.setenv("SAGE_HIP_DEBUG_FLAGS", str(flags))
    if clocks:
        monkeypatch.setenv("SAGE_HIP_PHASE_CLOCKS", "1")
    scorer = Scorer(dev, params)  # (the variables are read here, once)
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    lib = L.load()
    inst = np.zeros(1, np.uint32)
    L.check(lib.sage_hip_debug_rescore_instance(scorer._h, L.as_ptr(inst, C.c_uint32)))
    assert int(inst[0]) == 0xFFFFFFFF, "no launch yet"
    gf, gc = scorer.score_resident(scorer.upload(batch))
    gf, gc = gf.copy(), gc.copy()
    L.check(lib.sage_hip_debug_rescore_instance(scorer._h, L.as_ptr(inst, C.c_uint32)))
    counters = None
    if clocks:
        heavy, routes = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
        L.check(lib.sage_hip_debug_heavy_counters(scorer._h, L.as_ptr(heavy, C.c_uint64)))
        L.check(lib.sage_hip_debug_heavy_routes(scorer._h, L.as_ptr(routes, C.c_uint64)))
        counters = (int(heavy[0]), int(heavy[1]), int(routes[0]), int(routes[1]))
    scorer.close()
    return gf, gc, int(inst[0]), counters


def records(gf, gc):
    return gc.tobytes() + gf[np.arange(gf.shape[1])[None, :] < gc[:, None]].tobytes()


def check(world, batch, expected, params, monkeypatch, ctx, two_kinds, general=False):
    """every flag set: the default choice of the instance and SAGE_HIP_RESCORE_KINDS_GENERAL=1 against each other and the oracle, and
    the debug call on which instance ran"""
    of, oc = expected
    base = None
    for flags in FLAG_SETS:
        gf, gc, inst, _ = run(world.dev, batch, params, monkeypatch, flags, general=general)
        assert not (inst & (INST_BIG | INST_PROF)), (ctx, flags, inst)
        assert bool(inst & INST_KINDS2) == two_kinds, f"{ctx}, flags={flags}: instance {inst:#x}"
        assert bool(inst & INST_CHIMERA) == (general or bool(params.chimera)), f"{ctx}, flags={flags}: instance {inst:#x}"
        n = assert_features_equal(gf, gc, of, oc, f"{ctx}, flags={flags}")
        if base is None:
            base = records(gf, gc)
            assert n > 0, ctx
        assert records(gf, gc) == base, f"{ctx}: flags={flags} changed the records"
        gf, gc, inst, _ = run(world.dev, batch, params, monkeypatch, flags, kinds_general=True, general=general)
        assert not (inst & INST_KINDS2), f"{ctx}, flags={flags}, SAGE_HIP_RESCORE_KINDS_GENERAL=1: instance {inst:#x}"
        assert records(gf, gc) == base, f"{ctx}, flags={flags}: the general instance's records differ"
    return base


PARAMS = dict(max_precursor_charge=6, max_fragment_charge=None)


@pytest.mark.parametrize("min_matched_peaks", [1, 4])
@pytest.mark.parametrize("name", sorted(TWO_KINDS))
def test_two_kind_databases(cases, monkeypatch, name, min_matched_peaks):
    """{b, y}, {c, z}, {a, x}: the two-kind instance; min_matched_peaks 1 (a lone match reports) and 4 (the prune drops candidates)"""
    c = cases(name)
    params = ScorerParams(min_matched_peaks=min_matched_peaks, **PARAMS)
    base = check(c.world, c.batch, c.expected(params), params, monkeypatch, f"{name}, min_matched_peaks={min_matched_peaks}", True)
    # the made spectra do what they were made for: every length and charge reports, spectra of one side only among them, and the
    # spectra without a fragment's peak report nothing
    of, oc = c.expected(params)
    what = c.what
    for plen in sorted({w[0] for w in what}):
        for z in (2, 3, 4, 5):
            hit = [i for i, w in enumerate(what) if w[0] == plen and w[1] == z and w[2] != "none" and oc[i] > 0]
            # (the fragment index leaves out the first two ions of a series, ion_series.rs:196-208: a peptide of fewer than five residues
            # is in the table and on no candidate list)
            assert hit or plen < 5 or (plen == 5 and min_matched_peaks > 1), (name, plen, z)
    if min_matched_peaks == 1:
        b_only = [i for i, w in enumerate(what) if w[2] == "n" and oc[i] > 0 and of[i, 0]["matched_peaks"] > 0 and of[i, 0]["longest_y"] == 0]
        y_only = [i for i, w in enumerate(what) if w[2] == "c" and oc[i] > 0 and of[i, 0]["matched_peaks"] > 0 and of[i, 0]["longest_b"] == 0]
        both = [i for i, w in enumerate(what) if w[2] == "both" and oc[i] > 0 and of[i, 0]["longest_b"] > 0 and of[i, 0]["longest_y"] > 0]
        assert len(b_only) > 10 and len(y_only) > 10 and len(both) > 10, (len(b_only), len(y_only), len(both))
    assert all(oc[i] == 0 for i, w in enumerate(what) if w[2] == "none"), name
    # the profiling instance, every candidate on the cooperative path from its first hit: the same records, chunks and matches
    # counted, one-trip and per-charge routes both
    gf, gc, inst, counters = run(c.world.dev, c.batch, params, monkeypatch, EVERY_HEAVY | FIRST_HIT, clocks=True)
    assert inst & INST_KINDS2 and inst & INST_PROF, hex(inst)
    assert records(gf, gc) == base, f"{name}: the profiling two-kind instance"
    print(f"{name}, min_matched_peaks={min_matched_peaks}: {c.batch.n} spectra, heavy (chunks, matches, one-trip, per-charge) {counters}")
    assert counters[0] > 0 and counters[1] > 0 and counters[2] > 0 and counters[3] > 0, counters
    gf, gc, inst, _ = run(c.world.dev, c.batch, params, monkeypatch, EVERY_HEAVY | FIRST_HIT, kinds_general=True, clocks=True)
    assert not (inst & INST_KINDS2) and inst & INST_PROF, hex(inst)
    assert records(gf, gc) == base, f"{name}: the profiling general instance"


@pytest.mark.parametrize("name", sorted(GENERAL))
def test_other_kind_lists_keep_the_general_instance(cases, monkeypatch, name):
    """{y, b}, {b}, {b, y, c}, six kinds: never the two-kind instance, whatever the variable says"""
    c = cases(name)
    params = ScorerParams(min_matched_peaks=1, **PARAMS)
    check(c.world, c.batch, c.expected(params), params, monkeypatch, name, False)


def test_chimera_and_the_general_switch_keep_the_general_instance(cases, monkeypatch):
    """{b, y} with chimera rounds, and with SAGE_HIP_RESCORE_GENERAL=1"""
    c = cases("by")
    chim = ScorerParams(chimera=True, report_psms=2, min_matched_peaks=2, **PARAMS)
    check(c.world, c.batch, c.expected(chim), chim, monkeypatch, "by, chimera", False)
    params = ScorerParams(min_matched_peaks=1, **PARAMS)
    check(c.world, c.batch, c.expected(params), params, monkeypatch, "by, SAGE_HIP_RESCORE_GENERAL=1", False, general=True)


def test_high_charges_in_c3_like_lists(high_charge_world, monkeypatch):
    """the high-charge world of test_gpu_rescore_heavy_adds.py: precursor charges 4, 5 and 6 — three filtered fragment charges, four and
    five unfiltered — in lists of several candidates"""
    w = high_charge_world
    assert {4, 5, 6} <= set(np.asarray(w.batch.precursor_charge).tolist())
    params = ScorerParams(**PARAMS)
    check(w, w.batch, w.orc.score(params, w.batch)[:2], params, monkeypatch, "charges 4 to 6", True)
