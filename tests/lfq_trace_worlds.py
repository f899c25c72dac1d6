"""Multi-page feature maps built so that named seams of the tracing pass are reached — TEST INFRASTRUCTURE, no test.

Six worlds, made without a database (a feature table, composition arrays, MS1 batches), whose window counts put the page
count of the feature map on both sides of a power of two (the page sort's key width is 32 + bits_for(n_pages)):

    world  features  charges  windows   pages
    p1       455      1-6      16 380   1, four short of full
    p2     2 731      2-2      16 386   2, the last page holds two windows
    p4     5 461      2-3      65 532   4
    p5     3 641      2-4      65 538   5, the last page holds two windows; ion mobility
    p8     4 369      1-5     131 070   8
    p9     3 641      1-6     131 076   9

Every calcmass lies in [800, 2400] and ppm <= 10, so every window is narrower than 0.05: lfq_trace_bruteforce accepts the map
(require_layout_free) and its brute force over all (peak, window) pairs defines every grid bit for bit.

What a world holds, from a fixed seed:
  - feature RTs in [0.40, 0.43], so a spectrum's +-0.005 covers several pages; forty features below 0.01, whose decoy windows
    clamp to rt 0; in p8 / p9 one rt on at least 2 * 16 384 forward windows, so two consecutive pages share a min_rt;
  - rows of the feature table that must not count: decoy PSMs, a more confident PSM above the q-value threshold, a later PSM
    of a peptide already taken;
  - 100-150 MS1 spectra of 150-300 peaks over n_files files, their peaks as given NOT in mass order, in at least three batches out of file
    order with an empty batch among them; empty spectra first, last and two adjacent;
  - spectrum RTs through alignments with slope != 1, intercept != 0, max_rt != 1: one exactly on every page's min_rt, one
    that looks just below a page's min_rt and far past it, for the shared min_rt one with f32(rt - RT_TOL) == min_rt and one
    with f32(rt + RT_TOL) == min_rt, some near 0, the rest drawn;
  - peaks aimed at windows whose rt passes for the spectrum, at least two in every page the spectrum looks into: the centre,
    exactly mass_lo, exactly mass_hi, and one ulp outside each (dropped if another window happens to lie there: they must
    match nothing); on every seam both windows beside it, which but for some seams 3, 6 belong to one feature; noise; duplicated m/z with other
    intensities; intensities from a lognormal with sigma 3, some 0.0 (in the clusters below every other one times
    2^40: a cell's f64 sum of a few f32 values is exact, and so the same in any order, until they lie more than 2^29 apart);
  - p5: mobilities inside the window, exactly on its bounds and one ulp outside; every third spectrum of file 1 has no
    mobility column;
  - two clusters of nine spectra at nearly one RT each, aimed at one window each of 110 features (220 in all): their cells
    receive many additions of unlike magnitude;
  - a spectrum of the last file aimed at the decoy window of the highest peptide, highest charge, third isotope: the last
    row of the last grid slot.

`census` asserts all of this from the brute force's matches.  The pages it speaks of are those of a stable sort by rt of the
windows in (peptide, charge, isotope, decoy) order cut every 16 384: where rts tie across a seam another sort may cut
elsewhere (the matches do not depend on it), and tests/test_lfq_trace_cpu.py checks that the restatement's pages are these."""
import numpy as np

import lfq_trace_bruteforce as B
from lfq_traces import mz_for_mass
from sage_amd import _lib as L
from sage_amd.api import ALIGNMENT_DTYPE, RawBatch, RawSpectrum, peptide_compositions

F32 = np.float32
PAGE = 16 * 1024      # lfq.rs:176, :190 — the census's, never the brute force's
UP, DOWN = F32(np.inf), F32(-np.inf)
RESIDUES = np.frombuffer(b"ARNDCEQGHILKMFPSTWYV", dtype=np.uint8)

#            features, charges, combine, files, ppm, ion mobility, pct, shared rt, seed, drawn spectra
SPECS = {
    "p1": dict(S=455, charge=(1, 6), combine=True, n_files=1, ppm=5.0, im=False, pct=1.0, shared=False, seed=9101, drawn=78),
    "p2": dict(S=2731, charge=(2, 2), combine=False, n_files=2, ppm=10.0, im=False, pct=1.0, shared=False, seed=9102, drawn=77),
    "p4": dict(S=5461, charge=(2, 3), combine=False, n_files=1, ppm=2.0, im=False, pct=1.0, shared=False, seed=9104, drawn=73),
    "p5": dict(S=3641, charge=(2, 4), combine=True, n_files=3, ppm=10.0, im=True, pct=1.5, shared=False, seed=9105, drawn=71),
    "p8": dict(S=4369, charge=(1, 5), combine=True, n_files=2, ppm=5.0, im=False, pct=1.0, shared=True, seed=9108, drawn=65),
    "p9": dict(S=3641, charge=(1, 6), combine=True, n_files=1, ppm=10.0, im=False, pct=1.0, shared=True, seed=9109, drawn=63),
}
WINDOWS = {"p1": 16380, "p2": 16386, "p4": 65532, "p5": 65538, "p8": 131070, "p9": 131076}
PAGES = {"p1": 1, "p2": 2, "p4": 4, "p5": 5, "p8": 8, "p9": 9}
NAMES = tuple(SPECS)
SHARED_RT = F32(0.4151)
N_LOW, N_DENSE, N_DENSE_SPECTRA = 40, 220, 9     # (dense spectra per centre)
_WORLDS = {}


class Sequences:
    """what lfq_traces.isotopes_of asks of a database: sequence(p)"""

    def __init__(self, seq_off, seq):
        self.seq_off, self.seq = seq_off, seq

    def sequence(self, p):
        return bytes(self.seq[int(self.seq_off[p]):int(self.seq_off[p + 1])]).decode()


def settings_of(name):
    import lfq_reference as R
    sp = SPECS[name]
    return R.default_settings(ppm_tolerance=sp["ppm"], mobility_pct_tolerance=sp["pct"], combine_charge_states=sp["combine"])


def sst_for_rt(target, alignment):
    """an f32 scan start time whose aligned rt (lfq.rs:241) is exactly `target`, or None"""
    _, max_rt, slope, intercept = alignment
    s = F32((float(target) - float(intercept)) / float(slope) * float(max_rt))
    for _ in range(256):
        got = B.aligned_rt(s, alignment)
        if got == target:
            return s
        s = np.nextafter(s, UP if got < target else DOWN)
    return None


def _pages(w):
    """per window its page and position of the stable sort by rt (generation order re-keyed by peptide), and the min_rts"""
    order = np.lexsort((w["decoy"], w["isotope"], w["charge"], w["peptide"], w["rt"]))
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    return pos // PAGE, order, w["rt"][order[::PAGE]]


def _features(sp, rng):
    S = sp["S"]
    n_pep = 3 * S
    lens = rng.integers(7, 26, n_pep)
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    seq = RESIDUES[rng.integers(0, len(RESIDUES), int(seq_off[-1]))]
    carbon, sulfur = peptide_compositions(seq_off, seq)
    chosen = rng.choice(n_pep, S, replace=False)
    chosen[0] = n_pep - 1 if n_pep - 1 not in chosen else chosen[0]        # the composition arrays' last entry is used
    rt = rng.uniform(0.40, 0.43, S).astype(F32)
    if sp["shared"]:
        nz = sp["charge"][1] - sp["charge"][0] + 1
        rt[:-(-2 * PAGE // (nz * 3))] = SHARED_RT
    rt[S - N_LOW:] = rng.uniform(0.0005, 0.0095, N_LOW).astype(F32)
    calc = rng.uniform(800.0, 2400.0, S).astype(F32)
    ims = rng.uniform(0.6, 1.4, S).astype(F32)
    perm = rng.permutation(S)
    rows = []  # (peptide, label, calcmass, file, aligned_rt, peptide_q, ims) in confidence order
    others = np.setdiff1d(np.arange(n_pep), chosen)
    for j, k in enumerate(perm):
        p = int(chosen[k])
        fid = int(rng.integers(0, sp["n_files"]))
        if j % 400 == 3:    # a decoy PSM, of a peptide that is never selected and of one that is
            rows.append((int(others[j // 400]), -1, 1500.0, 0, 0.41, 0.0, 1.0))
            rows.append((p, -1, float(calc[k]) + 2.0, 0, 0.41, 0.0, 1.0))
        if j % 400 == 7:    # a more confident PSM above the threshold: skipped
            rows.append((p, 1, float(calc[k]) + 1.0, fid, float(rt[k]) + 0.004, 0.5, 1.0))
        rows.append((p, 1, float(calc[k]), fid, float(rt[k]), 0.001 * (j % 10), float(ims[k])))
        if j % 400 == 11:   # a later PSM of the same peptide: ignored
            rows.append((p, 1, float(calc[k]) + 3.0, (fid + 1) % sp["n_files"], 0.2, 0.0, 1.2))
    f = np.zeros(len(rows), dtype=L.FEATURE_DTYPE)
    f["peptide_idx"], f["label"] = [r[0] for r in rows], [r[1] for r in rows]
    f["calcmass"], f["file_id"], f["charge"] = [r[2] for r in rows], [r[3] for r in rows], 2
    f["ims"] = [r[6] for r in rows]
    art = np.array([r[4] for r in rows], F32)
    pq = np.array([r[5] for r in rows], F32)
    return f, art, pq, seq_off, seq, carbon, sulfur, int(chosen.max())


def _alignments(sp, rng):
    al = np.zeros(sp["n_files"], ALIGNMENT_DTYPE)
    for i in range(sp["n_files"]):
        al[i] = (i, F32(rng.uniform(400.0, 600.0)), F32(rng.uniform(0.8, 1.25)), F32(-rng.uniform(0.01, 0.05)))
    # File 0 carries the spectra whose aligned rt is asked for exactly.  Every f32 rt in [0.38, 0.44] is reachable when one ulp
    # of the scan start time moves each intermediate result by less than that result's own ulp: scan start times below 256
    # over a max_rt above 512 (a quotient below 0.5 in steps under 2^-25), a slope just below one, a small intercept.  The
    # intercept is minus the product of a scan start time of its own, so that rt 0.0 is reachable too.
    max_rt, slope = F32(rng.uniform(515.0, 545.0)), F32(rng.uniform(0.975, 0.999))
    sst0 = F32(rng.uniform(6.0, 10.0))
    al[0] = (0, max_rt, slope, -F32(F32(sst0 / max_rt) * slope))
    return al


class _Spectrum:
    def __init__(self, fid, sst, rt, kind):
        self.fid, self.sst, self.rt, self.kind = fid, F32(sst), F32(rt), kind
        self.mass, self.inten, self.mob, self.aim = [], [], [], []   # aim: (window, expect, what) per peak
        self.has_mob = True


def _aim(sp, w, page, s, rng, forced=(), n_more=24, per_page=2):
    """peaks of spectrum `s` aimed at windows whose rt passes: the forced ones, two of every page it looks into, n_more others"""
    lo, hi = F32(s.rt - B.RT_TOL), F32(s.rt + B.RT_TOL)
    passes = (w["rt"] <= hi) & (w["rt"] >= lo)
    near = np.flatnonzero(passes)
    targets = [int(t) for t in forced]
    assert passes[targets].all(), "a forced window's rt passes"
    for k in np.unique(page[near]) if per_page else ():
        here = near[page[near] == k]
        targets += [int(t) for t in rng.choice(here, min(per_page, len(here)), replace=False)]
    if len(near):
        targets += [int(t) for t in rng.choice(near, min(n_more, len(near)), replace=False)]
    targets = list(dict.fromkeys(targets))
    outside = []
    for t in targets:
        wlo, whi = w["mass_lo"][t], w["mass_hi"][t]
        centre = F32((wlo + whi) / F32(2.0))
        inside_mob = F32(1.0)
        if sp["im"]:
            mlo, mhi = w["mobility_lo"][t], w["mobility_hi"][t]
            inside_mob = F32(rng.uniform(float(np.nextafter(mlo, UP)), float(np.nextafter(mhi, DOWN))))
            for mob, ok, what in ((mlo, True, "mobility_lo"), (mhi, True, "mobility_hi"), (np.nextafter(mlo, DOWN), False, "below mobility_lo"),
                                  (np.nextafter(mhi, UP), False, "above mobility_hi")):
                if rng.random() < 0.25:
                    s.mass.append(centre), s.mob.append(F32(mob)), s.aim.append((t, ok, what))
        for m, ok, what in ((centre, True, "centre"), (wlo, True, "mass_lo"), (whi, True, "mass_hi"),
                            (np.nextafter(wlo, DOWN), False, "below mass_lo"), (np.nextafter(whi, UP), False, "above mass_hi")):
            if not ok:
                outside.append(len(s.mass))
            s.mass.append(F32(m)), s.mob.append(inside_mob), s.aim.append((t, ok, what))
    # an outside peak must match nothing: drop those that another window with a passing rt happens to hold
    if outside:
        m = np.array([s.mass[i] for i in outside], F32)[:, None]
        held = ((m >= w["mass_lo"][near][None, :]) & (m <= w["mass_hi"][near][None, :])).any(axis=1)
        for i in sorted((i for i, h in zip(outside, held) if h), reverse=True):
            del s.mass[i], s.mob[i], s.aim[i]
    return targets


def _finish(sp, s, rng, n_noise=40, n_dup=10, lift=False):
    """noise, duplicated m/z, intensities; the peaks as given in a drawn order (the port sorts them)"""
    n = len(s.mass)
    for _ in range(max(n_noise, 155 - n - (n_dup if n else 0))):      # (a spectrum that looks at few windows is filled up with noise)
        s.mass.append(F32(rng.uniform(130.0, 2500.0))), s.mob.append(F32(rng.uniform(0.5, 1.5))), s.aim.append((-1, None, "noise"))
    for i in rng.integers(0, max(n, 1), n_dup if n else 0):
        s.mass.append(s.mass[i]), s.mob.append(s.mob[i]), s.aim.append(s.aim[i][:2] + ("duplicate of " + s.aim[i][2],))
    mz = [mz_for_mass(F32(m)) for m in s.mass]
    keep = [i for i, v in enumerate(mz) if v is not None]
    order = rng.permutation(keep)
    s.mz = np.array([mz[i] for i in order], F32)
    s.mob = np.array([s.mob[i] for i in order], F32)
    s.aim = [s.aim[i] for i in order]
    s.inten = rng.lognormal(8.0, 3.0, len(order)).astype(F32)
    if lift:
        s.inten = (s.inten * np.where(rng.random(len(order)) < 0.5, F32(2.0 ** 40), F32(1.0))).astype(F32)
    s.inten[rng.random(len(order)) < 0.05] = F32(0.0)
    assert np.isfinite(s.inten).all() and 150 <= len(order) <= 300, len(order)


def _raw(sp, s, j):
    mob = s.mob if (sp["im"] and s.has_mob) else None
    return RawSpectrum(s.mz, s.inten, 0.0, None, None, float(s.sst), None, s.fid, f"{s.kind}-{j}", mobility=mob)


def _empty(sp, fid, sst):
    s = _Spectrum(fid, sst, 0.0, "empty")
    s.mz, s.inten, s.mob, s.aim = np.zeros(0, F32), np.zeros(0, F32), np.zeros(0, F32), []
    return s


def world(name):
    """the world `name`, built once: the device's inputs (f, art, pq, al, batches, carbon, sulfur), the brute force's (windows,
    spectra, alignments), what every peak was aimed at, and the layout the census speaks of"""
    if name in _WORLDS:
        return _WORLDS[name]
    sp = SPECS[name]
    rng = np.random.default_rng(sp["seed"])
    f, art, pq, seq_off, seq, carbon, sulfur, pmax = _features(sp, rng)
    w = B.build_windows(f["peptide_idx"], f["label"], f["calcmass"], art, pq, sp["charge"], sp["ppm"],
                        ims=f["ims"] if sp["im"] else None, mobility_pct=sp["pct"])
    B.require_layout_free(w)
    assert len(w["rt"]) == WINDOWS[name]
    page, order, min_rts = _pages(w)
    n_pages = len(min_rts)
    al = _alignments(sp, rng)
    alignments = [tuple(a) for a in al.tolist()]
    n_files = sp["n_files"]
    spectra = []

    def new(fid, rt, kind, exact=False):
        sst = sst_for_rt(F32(rt), alignments[fid])
        if sst is None:
            assert not exact, f"no scan start time of file {fid} aligns to {rt!r}"
            sst = F32((float(rt) - alignments[fid][3]) / alignments[fid][2] * alignments[fid][1])
        assert sst >= 0.0
        s = _Spectrum(fid, sst, B.aligned_rt(sst, alignments[fid]), kind)
        assert not exact or s.rt == F32(rt)
        spectra.append(s)
        return s

    # one spectrum exactly on every page's min_rt, aimed at that page's first window and, on a seam, at both its sides
    seams = []
    for k in range(n_pages):
        first = int(order[k * PAGE])
        forced = [first]
        if k:
            before = int(order[k * PAGE - 1])
            forced.append(before)
            # a feature's 3 * charges windows of one kind share an rt and lie together, and 16 384 k is a multiple of that
            # count only for some k that are multiples of 3: every other seam cuts through one feature's windows
            if w["feature"][before] == w["feature"][first] and w["decoy"][before] == w["decoy"][first]:
                seams.append((k, before, first))
        if k and min_rts[k] == min_rts[k - 1]:
            spectra[-1].kind += f"+{k}"
            _aim(sp, w, page, spectra[-1], rng, forced, n_more=0, per_page=0)
        else:
            _aim(sp, w, page, new(0, min_rts[k], f"page{k}", exact=True), rng, forced)
    # one that looks just below a page's min_rt and 0.0098 past it
    for k in range(1, n_pages - 1):
        _aim(sp, w, page, new(k % n_files, F32(min_rts[k] + F32(0.0049)), f"span{k}"), rng, n_more=16)
    shared_pages = [k for k in range(1, n_pages) if min_rts[k] == min_rts[k - 1] == SHARED_RT]
    if sp["shared"]:
        assert shared_pages, "two consecutive pages share the forward run's min_rt"
        assert ((w["rt"] == SHARED_RT) & ~w["decoy"]).sum() >= 2 * PAGE
        for sign, kind in ((F32(1.0), "shared-lo"), (F32(-1.0), "shared-hi")):   # f32(rt - RT_TOL) == min_rt, f32(rt + RT_TOL) == min_rt
            rt = F32(SHARED_RT + sign * B.RT_TOL)
            for _ in range(16):
                got = F32(rt - sign * B.RT_TOL)
                if got == SHARED_RT:
                    break
                rt = np.nextafter(rt, UP if got < SHARED_RT else DOWN)
            assert F32(rt - sign * B.RT_TOL) == SHARED_RT
            s = new(0, rt, kind, exact=True)
            on = np.flatnonzero((w["rt"] == SHARED_RT) & ~w["decoy"])
            _aim(sp, w, page, s, rng, [int(t) for t in rng.choice(on, 6, replace=False)])
    # near rt 0: the clamped decoy windows and the low features
    for j in range(4):
        _aim(sp, w, page, new(j % n_files, F32(rng.uniform(0.001, 0.009)), "low"), rng)
    # the last row of the last grid slot
    zmax = sp["charge"][1]
    last = int(np.flatnonzero((w["peptide"] == pmax) & (w["charge"] == zmax) & (w["isotope"] == 2) & w["decoy"])[0])
    _aim(sp, w, page, new(n_files - 1, F32(w["rt"][last] + F32(0.0011)), "last-slot"), rng, [last])
    # drawn ones
    for j in range(sp["drawn"]):
        _aim(sp, w, page, new(int(rng.integers(0, n_files)), F32(rng.uniform(0.385, 0.435)), "drawn"), rng)
    for s in spectra:
        _finish(sp, s, rng)
    # the dense clusters: per centre one forward window each of N_DENSE / 2 features, and spectra within two bins of it
    for centre in ((SHARED_RT, F32(0.4251)) if sp["shared"] else (F32(0.4101), F32(0.4201))):
        fwd = np.flatnonzero(~w["decoy"] & (np.abs(w["rt"] - centre) < 0.0045))
        feats = np.unique(w["feature"][fwd])
        assert len(feats) >= N_DENSE // 2, len(feats)
        dense = [int(rng.choice(fwd[w["feature"][fwd] == ft])) for ft in rng.choice(feats, N_DENSE // 2, replace=False)]
        for j in range(N_DENSE_SPECTRA):
            s = new(j % n_files, F32(centre + F32(rng.uniform(-0.00005, 0.00005))), "dense")
            for t in dense:
                m = F32(rng.uniform(float(w["mass_lo"][t]), float(w["mass_hi"][t])))
                mob = F32((w["mobility_lo"][t] + w["mobility_hi"][t]) / F32(2.0)) if sp["im"] else F32(1.0)
                s.mass.append(m), s.mob.append(mob), s.aim.append((t, True, "dense"))
            _finish(sp, s, rng, n_noise=20, n_dup=30, lift=True)
    rng.shuffle(spectra)
    # p5: every third spectrum of file 1 has no mobility column
    if sp["im"]:
        for j, s in enumerate([s for s in spectra if s.fid == 1]):
            s.has_mob = j % 3 != 0
    # empty spectra first, last and two adjacent; file 0 in three batches, out of file order, an empty batch among them
    per_file = [[s for s in spectra if s.fid == fid] for fid in range(n_files)]
    t0 = per_file[0][0].sst
    mid = len(per_file[0]) // 2
    per_file[0] = per_file[0][:mid] + [_empty(sp, 0, t0), _empty(sp, 0, t0)] + per_file[0][mid:]
    a, b = len(per_file[0]) // 3, 2 * len(per_file[0]) // 3
    parts = [per_file[0][b:]] + per_file[1:][::-1] + [[]] + [per_file[0][:a], per_file[0][a:b]]
    parts[0] = [_empty(sp, 0, t0)] + parts[0]
    parts[-1] = parts[-1] + [_empty(sp, 0, t0)]
    given = [s for part in parts for s in part]
    batches = [RawBatch([_raw(sp, s, j) for j, s in enumerate(part)]) for part in parts]
    assert sum(1 for b in batches if b.n) >= 3 and any(b.n == 0 for b in batches)
    assert 100 <= sum(1 for s in given if len(s.mz)) <= 150, sum(1 for s in given if len(s.mz))
    out = dict(name=name, spec=sp, f=f, art=art, pq=pq, al=al, batches=batches, carbon=carbon, sulfur=sulfur, alignments=alignments,
               windows=w, page=page, order=order, min_rts=min_rts, seams=seams, shared_pages=shared_pages, given=given, last=last,
               pmax=pmax, db=Sequences(seq_off, seq), spectra=B.read_spectra(batches), n_files=n_files, cache={})
    _WORLDS[name] = out
    return out


def brute(wd, subset=None, prune=False):
    """the brute force's reading of the world (or of the spectra at positions `subset`), once; prune: by match_pruned"""
    key = (None if subset is None else tuple(subset), prune)
    if key not in wd["cache"]:
        spectra = wd["spectra"] if subset is None else [wd["spectra"][i] for i in subset]
        wd["cache"][key] = B.trace(wd["windows"], spectra, wd["alignments"], wd["n_files"], wd["spec"]["combine"], prune=prune)
    return wd["cache"][key]


def seam_spectra(wd):
    """positions of the spectra that sit on a page's min_rt, look across one, or sit a tolerance from the shared one"""
    return [i for i, s in enumerate(wd["given"]) if s.kind.startswith(("page", "span", "shared"))]


def census(wd):
    """The world's conditions, asserted on the brute force's matches alone.  Returns the figures."""
    name, sp, w, page = wd["name"], wd["spec"], wd["windows"], wd["page"]
    grids, n_matches, m = brute(wd)
    given = wd["given"]
    n_pages = len(wd["min_rts"])
    assert n_pages == PAGES[name] == -(-len(w["rt"]) // PAGE)
    if name in ("p2", "p5"):
        assert len(w["rt"]) - (n_pages - 1) * PAGE == 2, "the last page holds two windows"
    hit_pages = np.unique(page[m["window"]])
    assert hit_pages.tolist() == list(range(n_pages)), f"every page holds a matched window: {hit_pages.tolist()}"
    triples = set(zip(m["spectrum"].tolist(), m["raw_peak"].tolist(), m["window"].tolist()))
    pairs = set(zip(m["spectrum"].tolist(), m["raw_peak"].tolist()))
    # what every aimed peak must do
    n_bounds = n_outside = n_mob_outside = 0
    for i, s in enumerate(given):
        for j, (t, expect, what) in enumerate(s.aim):
            if expect is None:
                continue
            if what.endswith(("mobility_lo", "mobility_hi")) and not expect and not s.has_mob:
                expect = True      # without the column the mobility is not asked
            if expect:
                assert (i, j, t) in triples, (name, s.kind, what)
                n_bounds += what.endswith(("mass_lo", "mass_hi", "mobility_lo", "mobility_hi"))
            elif "mobility" in what:
                assert (i, j, t) not in triples, (name, s.kind, what)
                n_mob_outside += 1
            else:
                assert (i, j) not in pairs, (name, s.kind, what)
                n_outside += 1
    assert n_bounds >= 200 and n_outside >= 100, (n_bounds, n_outside)
    if sp["im"]:
        assert n_mob_outside >= 50 and any(not s.has_mob and len(s.mz) for s in given)
    # every seam that cuts a feature: both windows beside it are matched
    matched = np.zeros(len(w["rt"]), bool)
    matched[m["window"]] = True
    for k, before, first in wd["seams"]:
        assert matched[before] and matched[first] and page[before] == k - 1 and page[first] == k, f"seam {k}"
    assert len(wd["seams"]) >= n_pages - 1 - (n_pages - 1) // 3, "every seam k cuts one feature's windows, but for some k that are multiples of 3"
    # one spectrum whose matches lie in three or more pages
    widest = 0
    for i in np.unique(m["spectrum"]):
        widest = max(widest, len(np.unique(page[m["window"][m["spectrum"] == i]])))
    if n_pages >= 4:
        assert widest >= 3, widest
    # the spectra on every page's min_rt, and a tolerance from the shared one, have matches
    for i, s in enumerate(given):
        if s.kind.startswith(("page", "shared")):
            assert (m["spectrum"] == i).any(), s.kind
    kinds = {s.kind for s in given}
    if sp["shared"]:
        assert {"shared-lo", "shared-hi"} <= kinds and wd["shared_pages"]
    # the low features' decoy windows clamp to rt 0, and are matched
    assert ((w["rt"] == 0) & w["decoy"]).sum() == N_LOW * (sp["charge"][1] - sp["charge"][0] + 1) * 3
    assert (w["rt"][m["window"]] == 0).any(), "a clamped decoy window is matched"
    # cells with three or more additions, where the order shows
    keys, cell, value = B.additions(w, m, wd["n_files"], sp["combine"])
    n_cells = len(keys) * wd["n_files"] * 3 * B.GRID_SIZE
    acc, count = B.fold(cell, value, n_cells)
    rev, _ = B.fold(cell, value, n_cells, reverse=True)
    busy = count >= 3
    differ = busy & (acc.view(np.uint64) != rev.view(np.uint64))
    assert busy.sum() >= 50 and differ.sum() >= 50, (int(busy.sum()), int(differ.sum()))
    # the highest slot and its last row
    zkey = 0 if sp["combine"] else sp["charge"][1]
    assert keys[-1] == (wd["pmax"], zkey, True) and wd["pmax"] == int(w["peptide"].max()) == len(wd["carbon"]) - 1
    rows = wd["n_files"] * 3
    assert count.reshape(len(keys), rows, B.GRID_SIZE)[-1, rows - 1].sum() > 0, "the last row of the last slot"
    assert sorted(grids) == keys
    return dict(windows=len(w["rt"]), pages=n_pages, spectra=len(given), peaks=int(sum(len(s.mz) for s in given)), matches=n_matches,
                grids=len(keys), widest=widest, busy_cells=int(busy.sum()), order_shows=int(differ.sum()), most=int(count.max()),
                bounds=n_bounds, outside=n_outside)
