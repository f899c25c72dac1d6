"""One scorer handle across sequences of different steps: the world, the named batches, the oracle cache and the step alphabet of
tests/test_gpu_handle_sequences.py (needs a device) and tests/test_handle_sequences_cpu.py (does not; it holds the world to what
the GPU tests rest on).

World: the isoleucine / leucine twin proteome of test_gpu_parity.test_equal_hyperscores_take_the_exact_path (a synthetic proteome
plus its I<->L mirror, bucket_size 1024, one missed cleavage) and a block of long proteins without I or L whose peptides — 45 to
50 heavy residues each, a fixed distance apart in mass — are heavier than every peptide of the twins.  Methionine oxidation is
variable, so that peptides with two methionines have positional isomers and the candidate lists the command line makes
(cli.isomer_candidates, cli.localisation_candidates) are not empty; peptide_max_mass is raised to make room for the block.

Every batch is a list of indices into ONE batch of unique spectra (`World.uniq`: 300 of twin peptides, 600 of the heavy block), so
the oracle scores a unique spectrum once per scorer configuration and a tiled batch's records are a gather with spec_index
rewritten (`World.oracle`; test_handle_sequences_cpu checks the gather against the oracle on the tiled batch itself)."""
import ctypes as C
import os
import types

import numpy as np

import oracle_lib
from parity_utils import assert_features_equal, assert_initial_hits_equal
from sage_amd import _lib as L
from sage_amd.api import DatabaseParameters, RawBatch, Scorer, ScorerParams, SpectrumBatch, SpectrumProcessor, Tolerance
from sage_amd.cli import isomer_candidates, localisation_candidates
from sage_amd.synthetic import _MASS, H2O, synthetic_fasta, synthetic_spectra

# the two scorer configurations (test_gpu_parity.py: n_retry > 50 on 300 twin spectra under the first, n_wide > 0 under the second)
CONFIGS = {
    "main": ScorerParams(report_psms=2, precursor_tol=Tolerance("da", -20.0, 20.0)),
    "second": ScorerParams(report_psms=3, precursor_tol=Tolerance("da", -200.0, 200.0)),
}
# batches scored under each configuration
BATCHES_OF = {"main": ("R", "Q", "Q2", "E", "S1", "S65", "BIG", "BIGQ"), "second": ("W", "N", "BIG")}
N_BIG = 24576
HEAVY_LO, HEAVY_HI, HEAVY_STEP = 6900.0, 8200.0, 26.0  # target masses of the heavy block's peptides
N_TWIN_SPECTRA, N_HEAVY_SPECTRA = 300, 600
MAX_PEAKS, DEISOTOPE = 150, True


def trim_k(params):
    """what trim_hits keeps of a preliminary list (scoring.rs: max(50, 2 * report_psms))"""
    return max(50, 2 * params.report_psms)


def heavy_fasta(seed=53):
    """Proteins of ten tryptic peptides each, no I / L / M / C / P inside: 44 to 49 residues of a W-rich alphabet and a lysine,
    the peptide nearest to each target mass out of 300 drawn ones.  Two neighbours together exceed 50 residues, so a missed
    cleavage adds no peptide."""
    rng = np.random.default_rng(seed)
    light = "DEFHNQY"
    peptides = []
    for target in np.arange(HEAVY_LO, HEAVY_HI, HEAVY_STEP):
        best = None
        for _ in range(300):
            n = int(rng.integers(44, 50))
            mean = (target - H2O - _MASS["K"]) / n  # the mean residue mass that reaches the target
            mean_light = float(np.mean([_MASS[c] for c in light]))
            p_w = float(np.clip((mean - mean_light) / (_MASS["W"] - mean_light), 0.05, 0.95))
            seq = "".join("W" if rng.random() < p_w else light[int(rng.integers(len(light)))] for _ in range(n)) + "K"
            mass = sum(_MASS[c] for c in seq) + H2O
            if best is None or abs(mass - target) < abs(best[0] - target):
                best = (mass, seq)
        peptides.append(best[1])
    out = []
    for p in range(0, len(peptides), 10):
        seq = "".join(peptides[p:p + 10])
        out.append(f">sp|HVY{p // 10:04d}|HVY{p // 10:04d}_SYNTH heavy block {p // 10}\n")
        out += [seq[j:j + 60] + "\n" for j in range(0, len(seq), 60)]
    return "".join(out)


def _only(host, chosen):
    """`host` as synthetic_spectra reads it, with only the `chosen` peptides as targets to draw from"""
    return types.SimpleNamespace(decoy=np.where(chosen, host.decoy, 1).astype(np.uint8), seq_off=host.seq_off, seq=host.seq,
                                 mods=host.mods, nterm=host.nterm, pep_mono=host.pep_mono, n_peptides=host.n_peptides)


def neutral_mass(batch):
    """the mass a known-charge spectrum's precursor window is centred on (scoring.rs: (m/z - proton) * charge), in f64"""
    return (batch.precursor_mz.astype(np.float64) - 1.0072764) * batch.precursor_charge.astype(np.float64)


class World:
    def __init__(self):
        fasta = synthetic_fasta(60, seed=17)
        twin = fasta.replace("I", "#").replace("L", "I").replace("#", "L").replace(">sp|SYN", ">sp|TWN")
        self.db_params = DatabaseParameters(bucket_size=1024, enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                                            static_mods={"C": 57.0215}, variable_mods={"M": [15.9949]}, peptide_max_mass=8400.0)
        self.host = self.db_params.build(fasta + twin + heavy_fasta())
        self.orc = oracle_lib.OracleDb.from_product(self.host)
        self.heavy = np.array(["HVY" in self.host.peptide_proteins(i) for i in range(self.host.n_peptides)])
        self.groups = self.host.isomer_groups()
        self.raw_twin = synthetic_spectra(_only(self.host, ~self.heavy), N_TWIN_SPECTRA, seed=29)
        self.raw_heavy = synthetic_spectra(_only(self.host, self.heavy), N_HEAVY_SPECTRA, seed=31)
        self.raw = self.raw_twin + self.raw_heavy
        sp = SpectrumProcessor(MAX_PEAKS, DEISOTOPE, 0.0)
        self.uniq = SpectrumBatch.from_spectra([sp.process(r) for r in self.raw])
        r = np.arange(N_TWIN_SPECTRA, dtype=np.int64)
        h = N_TWIN_SPECTRA + np.arange(N_HEAVY_SPECTRA, dtype=np.int64)
        q, q2 = h[:300], h[300:]
        i = np.arange(N_BIG, dtype=np.int64)
        k65 = np.arange(65, dtype=np.int64)
        self.index = {
            "R": r, "Q": q, "Q2": q2, "E": np.zeros(0, np.int64), "S1": r[7:8],
            "S65": np.where(k65 % 2 == 1, r[(k65 * 3) % len(r)], q[(k65 * 5) % len(q)]),
            # a quarter from R (every fourth position), the rest from Q, both walked round and round
            "BIG": np.where(i % 4 == 0, r[(i // 4) % len(r)], q[(i - i // 4) % len(q)]),
            "BIGQ": q[i % len(q)],
            "W": r[::3], "N": h[1::3],
        }
        self._batches, self._oracle, self._uniq_oracle = {}, {}, {}

    def batch(self, name) -> SpectrumBatch:
        if name not in self._batches:
            self._batches[name] = self.uniq.subset(self.index[name])
        return self._batches[name]

    def raw_batch(self, name) -> RawBatch:
        return RawBatch([self.raw[int(i)] for i in self.index[name]])

    def window_counts(self, cfg, name):
        """peptides inside each spectrum's precursor window, from the host's peptide masses and the scorer's window widened by a
        part in a million of the mass (more than the f32 rounding of either side)"""
        tol = CONFIGS[cfg].precursor_tol
        assert tol.kind == "da"
        m = neutral_mass(self.batch(name))
        mono = np.sort(self.host.pep_mono.astype(np.float64))
        slack = 1e-6 * m + 1e-3
        return np.searchsorted(mono, m + tol.hi + slack, "right") - np.searchsorted(mono, m + tol.lo - slack, "left")

    def oracle_unique(self, cfg):
        """(features, counts) of the unique spectra that some batch of the configuration holds; nothing for the others"""
        if cfg not in self._uniq_oracle:
            params = CONFIGS[cfg]
            used = np.unique(np.concatenate([self.index[b] for b in BATCHES_OF[cfg]]))
            f = np.zeros((self.uniq.n, params.report_psms), dtype=L.FEATURE_DTYPE)
            c = np.zeros(self.uniq.n, np.uint32)
            of, oc, _, _ = self.orc.score(params, self.uniq.subset(used))
            f[used], c[used] = of, oc
            self._uniq_oracle[cfg] = (f, c, used)
        return self._uniq_oracle[cfg]

    def oracle(self, cfg, name):
        """the oracle's (features, counts) of a named batch: a gather of oracle_unique, spec_index rewritten"""
        key = (cfg, name)
        if key not in self._oracle:
            assert name in BATCHES_OF[cfg]
            f, c, _ = self.oracle_unique(cfg)
            idx = self.index[name]
            of, oc = f[idx].copy(), c[idx].copy()
            of["spec_index"] = np.arange(len(idx), dtype=np.uint32)[:, None]
            of.flags.writeable = oc.flags.writeable = False
            self._oracle[key] = (of, oc)
        return self._oracle[key]

    def oracle_keep(self, cfg, name, low_memory):
        key = (cfg, name, "keep", bool(low_memory))
        if key not in self._oracle:
            self._oracle[key] = self.orc.quick_score(CONFIGS[cfg], self.batch(name), bool(low_memory))
        return self._oracle[key]

    def oracle_annotation(self, cfg, name):
        key = (cfg, name, "annotate")
        if key not in self._oracle:
            self._oracle[key] = self.orc.annotate(CONFIGS[cfg], self.batch(name))
        return self._oracle[key]


_world = None


def world() -> World:
    """built once per process"""
    global _world
    if _world is None:
        _world = World()
    return _world


# ---- steps (these need a device) ---------------------------------------------------------------------------------------------
def valid_bytes(feats, counts):
    """the bytes of the records that hold a PSM, and of the counts"""
    feats = np.asarray(feats)
    return feats[np.arange(feats.shape[1])[None, :] < np.asarray(counts)[:, None]].tobytes() + np.asarray(counts).tobytes()


def candidate_calls(w, scorer, dbatch, feats, counts):
    """score_candidates and localise over the lists the command line makes (cli.search_file): (candidates, bytes, bytes)"""
    off, pep = isomer_candidates(w.groups, feats, counts)
    iso = scorer.score_candidates(dbatch, feats, counts, off, pep)
    loff, lpep = localisation_candidates(w.groups, feats, counts)
    loc = scorer.localise(dbatch, feats, counts, loff, lpep)
    return int(off[-1]), iso.tobytes(), loc.tobytes()


class Fresh:
    """What a fresh handle's FIRST step on a batch reports — it always launches its retry pass — and its candidate calls, measured
    once per (configuration, batch, parts asked for through SAGE_HIP_WAYS) and kept."""

    def __init__(self, w, dev):
        self.w, self.dev, self.kept = w, dev, {}

    def __call__(self, cfg, name):
        key = (cfg, name, os.environ.get("SAGE_HIP_WAYS"))
        if key not in self.kept:
            w = self.w
            s = Scorer(self.dev, CONFIGS[cfg])
            batch = w.batch(name)
            dbatch = s.upload(batch)
            gf, gc = s.score_resident(dbatch)
            gf, gc = gf.copy(), gc.copy()
            t = s.last_timing()
            assert_features_equal(gf, gc, *w.oracle(cfg, name), f"fresh handle, {name}")
            out = {k: t[k] for k in ("n_retry", "n_launches", "n_wide", "n_ways")}
            out["candidates"] = candidate_calls(w, s, dbatch, gf, gc) if 0 < batch.n <= 1000 else None
            dbatch.close()
            s.close()
            self.kept[key] = out
        return self.kept[key]


class Handle:
    """One scorer handle and the steps of the alphabet on it.  Every step compares what it gets with the oracle (the candidate
    calls: with the same calls on a fresh handle), every resident scoring step its n_retry, n_wide and n_ways with a fresh
    handle's, and its total_ms with the timing interval that was set: 0 on a step without events, above 0 on one with."""

    def __init__(self, w, cfg, dev, fresh):
        self.w, self.cfg, self.dev, self.params, self.fresh = w, cfg, dev, CONFIGS[cfg], fresh
        self.scorer = Scorer(dev, self.params)
        self.every, self.calls = 1, 0  # (sage_hip_scorer_set_timing_interval: events on every `every`-th resident step)
        self.log, self.label = [], ""

    def clone(self):
        """continue on a clone of the handle (the original is released)"""
        self.scorer = self.scorer.clone()
        self.every, self.calls = 1, 0
        self.log.append(("clone", None))

    def fork(self, label):
        """a second Handle on a clone of this one's scorer; both stay in use"""
        other = Handle.__new__(Handle)
        other.__dict__.update(self.__dict__)
        other.scorer, other.every, other.calls, other.log, other.label = self.scorer.clone(), 1, 0, [], label
        return other

    def timing(self, every):
        self.scorer.set_timing_interval(every)
        self.every, self.calls = every, 0
        self.log.append(("timing", every))

    def _resident(self, dbatch, n, pageable=False):
        s, rp = self.scorer, self.params.report_psms
        timed = self.every != 0 and self.calls % self.every == 0
        self.calls += 1
        if pageable:  # (Scorer.score_resident always hands page-locked arrays over)
            gf = np.zeros(max(n * rp, 1), dtype=L.FEATURE_DTYPE)
            gc = np.zeros(max(n, 1), dtype=np.uint32)
            L.check(L.load().sage_hip_score_resident(s._h, dbatch._h, gf.ctypes.data_as(C.c_void_p), L.as_ptr(gc, C.c_uint32)))
            gf, gc = gf[:n * rp].reshape(n, rp), gc[:n]
        else:
            gf, gc = s.score_resident(dbatch)
            gf, gc = gf.copy(), gc.copy()
        t = s.last_timing()
        t["timed"] = timed
        return gf, gc, t

    def step(self, kind, name):
        """One step on the batch `name`; returns last_timing() (and "records": the bytes of the step's records, "timed": whether
        the step had events) behind a resident scoring step, else None."""
        w, s = self.w, self.scorer
        self.log.append((kind, name))
        ctx = f"{self.label} step {len(self.log)} of {self.log}"
        batch = w.batch(name)
        if kind == "stream":
            gf, gc = s.score(batch)
            assert_features_equal(gf, gc, *w.oracle(self.cfg, name), ctx)
            return None  # (the streaming entry adds up its chunks' counters: not a resident step's figures)
        if kind == "process":  # raw spectra through the device's preprocessing, as the command line uploads a file
            dbatch, _ = s.process_upload(w.raw_batch(name), take_top_n=MAX_PEAKS, deisotope=DEISOTOPE, min_deisotope_mz=0.0, min_peaks=0)
        else:
            dbatch = s.upload(batch)
        try:
            if kind == "hits":
                assert_initial_hits_equal(s, dbatch, w.orc, self.params, batch, ctx)
                return None
            if kind in ("quick0", "quick1"):
                np.testing.assert_array_equal(s.quick_score(dbatch, kind == "quick1"), w.oracle_keep(self.cfg, name, kind == "quick1"),
                                              err_msg=ctx)
                return None
            if kind == "reupload":  # scored, closed, uploaded again
                gf, gc, _ = self._resident(dbatch, batch.n)
                assert_features_equal(gf, gc, *w.oracle(self.cfg, name), ctx + " (before the batch was closed)")
                dbatch.close()
                dbatch = s.upload(batch)
            gf, gc, t = self._resident(dbatch, batch.n, pageable=kind == "pageable")
            assert_features_equal(gf, gc, *w.oracle(self.cfg, name), ctx)
            want = self.fresh(self.cfg, name)
            assert t["n_retry"] == want["n_retry"], f"n_retry {t['n_retry']}, a fresh handle's {want['n_retry']}: {ctx}"
            assert t["n_wide"] == want["n_wide"] and t["n_ways"] == want["n_ways"], f"{t} against a fresh handle's {want}: {ctx}"
            if not t["timed"]:
                assert t["total_ms"] == 0.0, f"total_ms {t['total_ms']} on a step without events: {ctx}"
            elif batch.n:
                assert t["total_ms"] > 0.0, f"total_ms {t['total_ms']} on a step with events: {ctx}"
            if kind in ("annotate", "process") and batch.n:
                goff, garr = s.annotate(dbatch, gf, gc)
                ooff, oarr = w.oracle_annotation(self.cfg, name)
                np.testing.assert_array_equal(goff, ooff, err_msg=f"PSM offsets: {ctx}")
                for k in oarr:
                    np.testing.assert_array_equal(garr[k], oarr[k], err_msg=f"Fragments.{k}: {ctx}")
                t["annotation"] = goff.tobytes() + b"".join(garr[k].tobytes() for k in sorted(garr))
            if kind in ("candidates", "process") and batch.n:
                got = candidate_calls(w, s, dbatch, gf, gc)
                assert got == want["candidates"], f"score_candidates / localise differ from a fresh handle's: {ctx}"
                t["candidates"] = got
            t["records"] = valid_bytes(gf, gc)
            return t
        finally:
            dbatch.close()

    def run(self, steps):
        """(kind, batch) steps, ("timing", k) and ("clone", None); the list of what the steps returned"""
        out = []
        for kind, arg in steps:
            if kind == "timing":
                out.append(self.timing(arg))
            elif kind == "clone":
                out.append(self.clone())
            else:
                out.append(self.step(kind, arg))
        return out


def draw_sequence(seed, n_steps=14):
    """A sequence of the first configuration's alphabet: (kind, batch) steps, ("timing", k) and ("clone", None); BIG / BIGQ at
    most once, and only in the resident steps (the oracle of their keep arrays and annotations would be the cost of the test)."""
    rng = np.random.default_rng(seed)
    small = ["R", "Q", "Q2", "E", "S1", "S65"]
    kinds = ["pinned", "pinned", "pageable", "stream", "reupload", "annotate", "candidates", "hits", "quick0", "quick1"]
    big_at = int(rng.integers(0, n_steps)) if rng.random() < 0.7 else -1
    seq = []
    for k in range(n_steps):
        u = rng.random()
        if k == big_at:
            seq.append((["pinned", "pageable"][int(rng.integers(2))], ["BIG", "BIGQ"][int(rng.integers(2))]))
        elif u < 0.08:
            seq.append(("timing", int(rng.integers(0, 4))))
        elif u < 0.14:
            seq.append(("clone", None))
        else:
            kind = kinds[int(rng.integers(len(kinds)))]
            name = small[int(rng.integers(len(small)))]
            if name == "E" and kind not in ("pinned", "pageable", "stream", "reupload"):
                kind = "pinned"  # (an empty batch has no records to annotate and no lists to compare)
            seq.append((kind, name))
    return seq
