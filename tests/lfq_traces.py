"""Drawing a chosen grid matrix through MS1 peaks, and the named integration cases — TEST INFRASTRUCTURE, no test.

No entry point of the library takes a grid matrix.  A trace is drawn the way test_gpu_lfq.py's `edge` fixture places single
peaks: with the identity alignment (rt = scan_start_time) one selected feature per peptide fixes the grid (aligned_rt = r), and
bin k of file f receives one MS1 spectrum at F32(F32(r - RT_TOL) + F32(k) * step) with one peak per isotope in the middle of
that isotope's window, its intensity profile[k] * dist[iso] * (1 + skew * iso).  Whether f32 rounding puts a peak into bin k or
k - 1 does not matter — the restatement traces the same peaks — except for a peptide at r = RT_TOL: its grid starts at 0.0,
every spectrum time is F32(k) * step, add_entry finds interp == 0.0 and cell k receives the intensity unchanged.  The cases
that need bitwise ties sit there.

`draw` builds the device's inputs and the restatement's from {(charge, decoy, file): profile} per peptide; `case(db, name)`
builds a named world once, traces it with tests/lfq_reference.py, asserts the case's defining property on the restatement's own
matrix, dot products or result (a case that stops being what its name says fails there), and returns it.  Nothing here calls
the device.

Also here, shared by the CPU and the GPU modules: the helpers test_gpu_lfq.py builds its worlds with, and its synthetic run."""
import numpy as np

import lfq_reference as R
from sage_amd import _lib as L
from sage_amd.api import ALIGNMENT_DTYPE, DatabaseParameters, RawBatch, RawSpectrum, peptide_compositions
from sage_amd.lcms import synthetic_lcms
from sage_amd.synthetic import synthetic_fasta

F32 = np.float32
STEP = (R.RT_TOL * F32(2.0)) / F32(R.GRID_SIZE)
CHARGES = (2, 3)              # precursor_charge of every named case
THRESHOLDS = (0.70, 0.0)
ACOS_ULPS = 8                 # test_gpu_lfq.ULPS: how far the device's acos may lie from libm's


def database():
    return DatabaseParameters(enzyme=dict(missed_cleavages=1, cleave_at="KR", restrict="P"),
                              static_mods={"C": 57.0215}).build(synthetic_fasta(60, seed=11))


def features_table(db, rows):
    """rows: (peptide_idx, label, calcmass, file_id, aligned_rt, peptide_q) in confidence order"""
    f = np.zeros(len(rows), dtype=L.FEATURE_DTYPE)
    for i, (p, lab, cm, fid, _, _) in enumerate(rows):
        f[i]["peptide_idx"], f[i]["label"], f[i]["calcmass"], f[i]["file_id"], f[i]["charge"] = p, lab, cm, fid, 2
    art = np.array([r[4] for r in rows], np.float32)
    pq = np.array([r[5] for r in rows], np.float32)
    return f, art, pq


def ref_feats(f, art, pq):
    return dict(peptide_idx=f["peptide_idx"], label=f["label"], calcmass=f["calcmass"], file_id=f["file_id"],
                aligned_rt=art, peptide_q=pq)


def ref_spectra(batches):
    out = []
    for b in batches:
        for i in range(b.n):
            lo, hi = int(b.peak_off[i]), int(b.peak_off[i + 1])
            m, it = R.process_ms1(b.mz[lo:hi], b.intensities[lo:hi])
            out.append((int(b.file_id[i]), F32(b.scan_start_time[i]), m, it))
    return out


def isotopes_of(db):
    cache = {}

    def f(p):
        if p not in cache:
            cache[p] = R.peptide_isotopes(*R.composition(db.sequence(p)))
        return cache[p]
    return f


def mz_for_mass(target):
    """an f32 m/z whose (mz - PROTON) is exactly `target` (f32), or None"""
    mz = F32(target) + R.PROTON
    for _ in range(64):
        d = F32(mz - R.PROTON)
        if d == target:
            return mz
        mz = np.nextafter(mz, F32(np.inf) if d < target else F32(-np.inf))
    return None


def unit_alignments(n):
    al = np.zeros(n, ALIGNMENT_DTYPE)
    for i in range(n):
        al[i] = (i, 1.0, 1.0, 0.0)  # rt = scan start time exactly
    return al


def run_world(db):
    """the 3-file synthetic run of test_gpu_lfq.py (its `run` fixture)"""
    rng = np.random.default_rng(21)
    files = synthetic_lcms(db, n_files=3, n_peptides=30, ms1_per_file=400, seed=2, ms1_noise=40)
    peps, apex = files[0].peptides, files[0].apex
    rows = []
    others = np.flatnonzero(db.decoy != 0)[:5]
    for p in others:  # decoy PSMs first: never selected
        rows.append((int(p), -1, float(db.pep_mono[p]), 0, 0.5, 0.0))
    for k, p in enumerate(peps):
        fid = k % 3
        if k % 4 == 0:  # a more confident PSM above the threshold: skipped, the next one counts
            rows.append((int(p), 1, float(db.pep_mono[p]) + 1.0, fid, float(apex[k]) + 0.01, 0.5))
        rows.append((int(p), 1, float(db.pep_mono[p]), fid, float(apex[k] + rng.normal(0, 0.0003)), 0.001 * (k % 9)))
        if k % 5 == 0:  # a later confident PSM of the same peptide: ignored
            rows.append((int(p), 1, float(db.pep_mono[p]), (fid + 1) % 3, float(apex[k]) + 0.002, 0.0))
    f, art, pq = features_table(db, rows)
    T = 60.0
    al = np.zeros(3, ALIGNMENT_DTYPE)
    for i, lf in enumerate(files):
        al[i] = (i, F32(T), F32(1.0 / lf.rt_scale), F32(-lf.rt_shift / (T * lf.rt_scale)))
    batches = []
    for i, lf in enumerate(files):
        ms1 = [s for s, lvl in zip(lf.spectra, lf.ms_levels) if lvl == 1]
        if i == 1:  # decoy windows with signal (mass + 11.06 at rt - 0.01), so the precursor FDR has decoys to count
            for k in range(0, len(peps), 3):
                t = (float(apex[k]) - 0.01) * T * lf.rt_scale + lf.rt_shift
                for s in ms1:
                    if abs(s.scan_start_time - t) < 0.2:
                        bait = (float(db.pep_mono[peps[k]]) + np.arange(3) * 1.00335) / 2 + 11.06 + 1.0072764
                        s.mz = np.sort(np.concatenate([s.mz, bait.astype(np.float32)]))
                        s.intensity = np.concatenate([s.intensity, rng.lognormal(11.0, 1.0, 3).astype(np.float32)])
        if i == 0:  # an MS1 spectrum without peaks
            ms1.insert(10, RawSpectrum(np.zeros(0, np.float32), np.zeros(0, np.float32), 0.0, None, None, ms1[10].scan_start_time, None, 0, "empty"))
        batches.append(RawBatch(ms1))
    c, s = peptide_compositions(db.seq_off, db.seq)
    return dict(f=f, art=art, pq=pq, al=al, batches=batches, carbon=c, sulfur=s,
                spectra=ref_spectra(batches), alignments=[tuple(a) for a in al.tolist()], cache={})


# ---- drawing -------------------------------------------------------------------------------------------------------------------
def pick_peptides(db, n):
    """the first n target peptides of ascending index between 1 200 and 2 400 Da (isotope windows of z = 2 and 3 far apart)"""
    ok = np.flatnonzero((db.decoy == 0) & (db.pep_mono > 1200.0) & (db.pep_mono < 2400.0))
    assert len(ok) >= n
    return [int(p) for p in ok[:n]]


def draw(db, peptides, n_files, precursor_charge=CHARGES, skew=0.02, ppm=5.0):
    """peptides: a list of dict(traces={(charge, decoy, file): profile[100] or [3, 100]}, ref=reference file, r=aligned_rt or None,
    skew=...).  A [3, 100] profile gives every isotope its own row (a deliberately wrong pattern).  Returns the world: the device's
    inputs (f, art, pq, al, batches, carbon, sulfur), the restatement's (fmap, spectra, alignments), and per peptide its index."""
    idx = pick_peptides(db, len(peptides))
    if len(peptides) == 1 and peptides[0].get("peptide") is not None:
        idx = [int(peptides[0]["peptide"])]
    iso_of = isotopes_of(db)
    rows = []
    for j, (p, spec) in enumerate(zip(idx, peptides)):
        r = F32(spec["r"]) if spec.get("r") is not None else F32(0.2 + 0.1 * j)
        rows.append((p, 1, float(db.pep_mono[p]), int(spec["ref"]), float(r), 0.0))
    f, art, pq = features_table(db, rows)
    settings = R.default_settings(ppm_tolerance=ppm)
    fmap = R.build_feature_map(settings, precursor_charge, ref_feats(f, art, pq))
    window = {(e["peptide"], e["charge"], e["isotope"], e["decoy"]): e for e in fmap["ranges"]}
    spectra = {}   # (file, time) -> [(mz, intensity)]
    for p, spec, r in zip(idx, peptides, art):
        dist = iso_of(p)
        sk = spec.get("skew", skew)
        for (z, decoy, fid), profile in spec["traces"].items():
            assert 0 <= fid < n_files and precursor_charge[0] <= z <= precursor_charge[1]
            profile = np.asarray(profile, dtype=np.float64)
            per_iso = profile if profile.ndim == 2 else np.stack([profile * float(dist[i]) * (1.0 + sk * i) for i in range(3)])
            assert per_iso.shape == (3, R.GRID_SIZE)
            wins = [window[(p, z, iso, bool(decoy))] for iso in range(3)]
            mzs = [mz_for_mass(F32((w["mass_lo"] + w["mass_hi"]) / F32(2.0))) for w in wins]
            assert all(m is not None for m in mzs)
            assert all(w["rt"] == wins[0]["rt"] for w in wins)
            rt_min = F32(wins[0]["rt"] - R.RT_TOL)       # Grid::new: entry.rt - rt_tol (the decoy's rt is r - 2 RT_TOL, clamped)
            for k in range(R.GRID_SIZE):
                if not per_iso[:, k].any():
                    continue
                t = F32(rt_min + F32(k) * STEP)
                assert t >= 0.0 and abs(t - wins[0]["rt"]) <= R.RT_TOL, "a drawn bin lies outside the run or the window"
                peaks = spectra.setdefault((fid, float(t)), [])
                for iso in range(3):
                    if per_iso[iso, k] != 0.0:
                        peaks.append((mzs[iso], F32(per_iso[iso, k])))
    batches = []
    for fid in range(n_files):
        sp = []
        for (g, t) in sorted(k for k in spectra if k[0] == fid):
            peaks = spectra[(g, t)]
            assert len(peaks) <= 12
            mz = np.array([m for m, _ in peaks], np.float32)
            it = np.array([i for _, i in peaks], np.float32)
            order = np.argsort(mz, kind="stable")
            sp.append(RawSpectrum(mz[order], it[order], 0.0, None, None, t, None, fid, f"f{fid}t{t}"))
        assert len(sp) <= 100 * len(peptides) * 2
        if sp:
            batches.append(RawBatch(sp))
    al = unit_alignments(n_files)
    cc, ss = peptide_compositions(db.seq_off, db.seq)
    return dict(f=f, art=art, pq=pq, al=al, batches=batches, carbon=cc, sulfur=ss, fmap=fmap, spectra=ref_spectra(batches),
                alignments=[tuple(x) for x in al.tolist()], peptides=idx, n_files=n_files, charge=tuple(precursor_charge),
                ref={p: int(s["ref"]) for p, s in zip(idx, peptides)}, ppm=ppm,
                drawn_charges={z for s in peptides for (z, _, _) in s["traces"]})


def stages(grid, settings):
    """the restatement's own intermediate results of one grid, for the cases' assertions: the unwarped dot rows, the 151 warp
    dot products per file, the warps, the per-bin scores and spectral values on the warped traces"""
    dot, angle = R.summarize(grid, R.gaussian_kernel(0.5, R.K_WIDTH))
    dots = R.warp_dots(dot, grid["ref"])
    warps = R.find_time_warps(dot, grid["ref"])
    sc, spectral = R.scores(R.apply_time_warps(dot, warps), R.apply_time_warps(angle, warps), settings["peak_scoring"])
    return dict(dot=dot, angle=angle, dots=dots, warps=warps, scores=np.array(sc), spectral=np.array(spectral))


# ---- profiles --------------------------------------------------------------------------------------------------------------------
_K = np.arange(R.GRID_SIZE, dtype=np.float64)


def lobe(centre, width=4.0, height=2.0 ** 20, floor=2.0 ** -20):
    """a Gaussian lobe; cells below `floor` of the height are left empty (no spectrum is drawn for them)"""
    v = height * np.exp(-0.5 * ((_K - centre) / width) ** 2)
    return np.where(v >= height * floor, v, 0.0)


def steps(centre, values=(1, 2, 3, 2, 1), unit=2.0 ** 12):
    """small integers times a power of two around `centre`: bitwise the same wherever it is put"""
    v = np.zeros(R.GRID_SIZE)
    half = len(values) // 2
    v[centre - half:centre - half + len(values)] = np.array(values, dtype=np.float64) * unit
    return v


def only_third_isotope(profile):
    p = np.zeros((3, R.GRID_SIZE))
    p[2] = profile
    return p


def with_pattern(db_dist, profile, skew=0.02):
    return np.stack([np.asarray(profile) * float(db_dist[i]) * (1.0 + skew * i) for i in range(3)])


# ---- the named cases ---------------------------------------------------------------------------------------------------------------
def _st(scoring="Hybrid", thr=0.70, integration="Sum"):
    return R.default_settings(peak_scoring=scoring, spectral_angle=thr, integration=integration)


def _build_silent_file(db):
    w = draw(db, [dict(ref=0, traces={(2, False, 0): lobe(50), (2, False, 1): lobe(55, height=2.0 ** 19)})], 3)

    def check(w, grids):
        g = grids[True][(w["peptides"][0], 0, False)]
        s = stages(g, _st())
        assert not s["dot"][2].any() and not s["dots"][2].any(), "the dot-product row of file 2 is all zero"
        want = R.integrate(g, _st())
        assert want["warps"] == [0, 5, 75] and want["peak"] and want["areas"][2] == 0.0 and want["areas"][1] > 0.0
    return w, check


def _build_silent_reference(db):
    w = draw(db, [dict(ref=1, traces={(2, False, 0): lobe(50), (2, False, 2): lobe(40)})], 3)

    def check(w, grids):
        g = grids[True][(w["peptides"][0], 0, False)]
        s = stages(g, _st())
        assert g["ref"] == 1 and not s["dot"][1].any() and s["dot"][0].any() and s["dot"][2].any()
        assert not s["dots"].any(), "every offset of every file ties at 0.0"
        assert R.integrate(g, _st())["warps"] == [75, 75, 75]
    return w, check


_SHIFTS = ((74, 12), (75, 12), (-75, 87), (76, 11))  # (shift of file 1 against the reference, the reference's lobe)


def _build_large_shifts(db):
    w = draw(db, [dict(ref=0, traces={(2, False, 0): lobe(c, 3.0), (2, False, 1): lobe(c + s, 3.0, 2.0 ** 18)}) for s, c in _SHIFTS], 2)

    def check(w, grids):
        for p, (shift, c) in zip(w["peptides"], _SHIFTS):
            g = grids[True][(p, 0, False)]
            s = stages(g, _st())
            free = R.warp_dots(s["dot"], 0, slack=99)[1]   # the search without its slack
            assert int(np.argmax(free)) - 99 == shift, "the trace is shifted as named"
            want = R.integrate(g, _st())["warps"]
            assert want == [0, min(shift, 75)], (shift, want)
            if shift == 76:  # out of reach: the slack's last offset holds the largest dot product there is
                assert s["dots"][1][150] == s["dots"][1].max() > 0.0
    return w, check


def _build_tied_offsets(db):
    twin = steps(30) + steps(60)
    w = draw(db, [dict(ref=0, r=R.RT_TOL, traces={(2, False, 0): twin, (2, False, 1): steps(45, unit=2.0 ** 10)})], 2)

    def check(w, grids):
        g = grids[True][(w["peptides"][0], 0, False)]
        assert g["rt_min"] == 0.0
        d = stages(g, _st())["dots"][1]
        assert d[75 - 15] == d[75 + 15] == d.max() > 0.0 and (d == d.max()).sum() == 2, "`s_dots` has two equal maxima"
        assert R.integrate(g, _st())["warps"] == [0, 15], "the later of two equal offsets wins"
    return w, check


def _build_reference_file_2(db):
    w = draw(db, [dict(ref=2, traces={(2, False, 0): lobe(40, height=2.0 ** 18), (2, False, 1): lobe(65, height=2.0 ** 21),
                                      (2, False, 2): lobe(52)})], 3)

    def check(w, grids):
        g = grids[True][(w["peptides"][0], 0, False)]
        s = stages(g, _st())
        assert g["ref"] == 2 and s["warps"] == [-12, 13, 0]
        assert R.find_time_warps(s["dot"], 0) == [0, 25, 12], "file 0 as the reference gives other warps"
    return w, check


def _build_plateau(db):
    p = np.zeros(R.GRID_SIZE)
    p[15:85] = 2.0 ** 20
    w = draw(db, [dict(ref=0, traces={(2, False, 0): p})], 1)

    def check(w, grids):
        g = grids[True][(w["peptides"][0], 0, False)]
        for scoring in R.SCORING:
            st = _st(scoring)
            want, s = R.integrate(g, st), stages(g, st)
            above = s["scores"] >= want["score"] * 0.5
            run = max(len(r) for r in "".join("x" if a else " " for a in above).split())
            assert run >= 41, "at least 41 consecutive bins score >= best / 2"
            rt = want["rt"]
            if scoring in ("RetentionTime", "Hybrid"):  # (the other two choose their best bin among nearly equal ones)
                assert rt == 50
            if 35 <= rt < 65:
                assert (want["left"], want["right"]) == (rt - 20, rt + 20), (scoring, want)
                # the clamps stopped both walks: the bins they stopped on still pass both tests
                for b in (want["left"], want["right"]):
                    assert s["scores"][b] >= want["score"] * 0.5 and s["spectral"][b] >= 0.70
    return w, check


def _build_grid_ends(db):
    dist = isotopes_of(db)
    idx = pick_peptides(db, 6)

    def lone(p, k, spoiler):  # signal in bin k alone, and a strong third-isotope-only bin whose smoothing does not reach k
        a = np.zeros(R.GRID_SIZE)
        a[k] = 2.0 ** 20
        m = with_pattern(dist(p), a)
        m[2, spoiler] = 2.0 ** 34
        return m
    specs = []
    # file 1 is shifted inwards; file 2 is silent everywhere: its warp of +75 makes Sum read beyond bin 99 at the upper end
    # (no warp can reach below bin 0 from a peak at bin 0 or 1: that would take a lobe left of it)
    for c, other in ((0, 8), (1, 9), (98, 90), (99, 91)):
        specs.append(dict(ref=0, traces={(2, False, 0): lobe(c, 1.5), (2, False, 1): lobe(other, 1.5, 2.0 ** 22)}))
    specs.append(dict(ref=0, traces={(2, False, 0): lone(idx[4], 0, 5), (2, False, 1): lobe(3, 1.5)}))
    specs.append(dict(ref=0, traces={(2, False, 0): lone(idx[5], 99, 94), (2, False, 1): lobe(96, 1.5)}))
    w = draw(db, specs, 3)

    def check(w, grids):
        gs = [grids[True][(p, 0, False)] for p in w["peptides"]]
        st = _st("Intensity", 0.0)
        want = [R.integrate(g, st) for g in gs[:4]]
        assert all(x["peak"] for x in want) and [x["rt"] <= 2 for x in want] == [True, True, False, False]
        assert [x["rt"] >= 97 for x in want] == [False, False, True, True]
        assert all(x["warps"][2] == 75 and x["areas"][2] == 0.0 and x["areas"][1] > 0.0 for x in want)
        assert want[0]["left"] == 0 and want[0]["warps"][1] > 4 and want[1]["left"] == 0 and want[1]["warps"][1] > 4
        assert want[2]["right"] >= 99 and want[2]["warps"][1] < -4 and want[3]["right"] >= 99 and want[3]["warps"][1] < -4
        st = _st("SpectralAngle", 0.70)
        s0, s99 = stages(gs[4], st), stages(gs[5], st)
        assert (s0["spectral"][:10] >= 0.70).tolist() == [True] + [False] * 9, "of the first ten bins, bin 0 alone passes the threshold"
        assert (s99["spectral"][89:] >= 0.70).tolist() == [False] * 10 + [True], "of the last eleven, bin 99 alone"
        want = R.integrate(gs[4], st)
        assert (want["rt"], want["left"], want["right"]) == (0, 0, 1)
        want = R.integrate(gs[5], st)
        assert (want["rt"], want["left"], want["right"]) == (99, 98, 100), "right = best + 1 = 100 with rmax = 99"
        assert stages(gs[4], _st("Hybrid"))["scores"][0] == 0.0 and R.integrate(gs[4], _st("Hybrid"))["rt"] > 0, "bin 0 has rt_factor 0.0"
    return w, check


def _build_equal_scores(db):
    w = draw(db, [dict(ref=0, r=R.RT_TOL, traces={(2, False, 0): steps(30) + steps(60)})], 1)

    def check(w, grids):
        g = grids[True][(w["peptides"][0], 0, False)]
        st = _st("Intensity", 0.0)
        s, want = stages(g, st), R.integrate(g, st)
        top = s["scores"].max()
        hits = np.flatnonzero(s["scores"] == top)
        assert len(hits) == 2 and hits[1] - hits[0] == 30 and top == 1.0, "two bins with exactly equal score"
        assert want["rt"] == hits[0], "the first is kept"
    return w, check


def _build_threshold_stop(db):
    dist = isotopes_of(db)
    p = pick_peptides(db, 1)[0]
    good = lobe(50, 8.0)
    m = with_pattern(dist(p), np.where(_K < 60, good, 0.0))
    m[2] += np.where(_K >= 60, good * 64.0, 0.0)          # the right flank: only the third isotope
    w = draw(db, [dict(ref=0, traces={(2, False, 0): m})], 1)

    def check(w, grids):
        g = grids[True][(w["peptides"][0], 0, False)]
        st = _st("Intensity", 0.70)
        s, want = stages(g, st), R.integrate(g, st)
        r = want["right"]
        assert want["peak"] and want["rt"] + 2 < r < min(want["rt"] + 20, 99), "a walk of some bins, and not the clamp"
        assert s["scores"][r] >= want["score"] * 0.5 and s["spectral"][r] < 0.70, "the angle threshold stopped the walk, not the score"
        assert R.integrate(g, _st("Intensity", 0.0))["right"] > r
    return w, check


def _build_threshold_fails(db):
    w = draw(db, [dict(ref=0, traces={(2, False, 0): only_third_isotope(lobe(50)), (2, False, 1): only_third_isotope(lobe(47))})], 2)

    def check(w, grids):
        g = grids[True][(w["peptides"][0], 0, False)]
        assert stages(g, _st())["spectral"].max() < 0.70
        for scoring in R.SCORING:
            assert not R.integrate(g, _st(scoring))["peak"]
        assert R.integrate(g, _st("Intensity", 0.0))["peak"]
    return w, check


def exact_bins():
    """the bins k of a grid that starts at 0.0 whose spectrum time F32(k) * step add_entry puts into bin k with interp == 0.0
    (for the others floor((t - 0) / step) is k - 1 and the intensity is split)"""
    t = (np.arange(R.GRID_SIZE, dtype=np.float32) * STEP).astype(np.float32)
    return np.floor(t / STEP) == np.arange(R.GRID_SIZE)


def _build_proportional(above_one):
    """a trace exactly proportional to the isotope distribution.  Whether the similarity then rounds above 1.0 (acos gives NaN
    and no bin with signal qualifies) or below depends on the f32 rounding of the peptide's sqrt(sum of squares): one case each"""
    def build(db):
        prof = np.where(exact_bins() & (_K >= 30) & (_K < 70), 2.0 ** (20.0 - np.abs(_K - 50.0)), 0.0)
        assert (prof != 0.0).sum() >= 20
        iso_of = isotopes_of(db)

        def nan_bins(p):
            d = iso_of(p)
            _, angle = R.summarize(dict(matrix=np.stack([prof * float(d[i]) for i in range(3)]), dist=d), R.gaussian_kernel(0.5, R.K_WIDTH))
            return int(np.isnan(angle).sum())
        p = next(p for p in pick_peptides(db, 40) if (nan_bins(p) > 0) == above_one)
        w = draw(db, [dict(peptide=p, ref=0, r=R.RT_TOL, skew=0.0, traces={(2, False, 0): prof})], 1)

        def check(w, grids):
            g = grids[True][(w["peptides"][0], 0, False)]
            assert g["rt_min"] == 0.0
            for iso in range(3):
                assert np.array_equal(g["matrix"][iso], prof * float(g["dist"][iso])), "every cell is exactly profile x distribution"
            s = stages(g, _st())
            signal = s["dot"][0] > 0.0
            if above_one:
                assert np.isnan(s["angle"][0][signal]).all() and signal.sum() > 40, "sim rounds above 1.0 wherever there is signal"
                assert not any(R.integrate(g, _st(sc))["peak"] for sc in R.SCORING)
            else:
                assert not np.isnan(s["angle"]).any() and s["angle"][0][signal].min() > 0.999
                assert all(R.integrate(g, _st(sc))["peak"] for sc in R.SCORING)
        return w, check
    return build


def _shifted_files(n, ref):
    shift = [((f * 5) % n - n // 2) * 4 for f in range(n)]
    return shift, {(2, False, f): lobe(50 + shift[f], 3.0 + 0.5 * f, 2.0 ** (14 + f) * (1 + 2 * (f % 3))) for f in range(n)}


def _build_files(n, ref):
    def build(db):
        shift, traces = _shifted_files(n, ref)
        w = draw(db, [dict(ref=ref, traces=traces)], n)

        def check(w, grids):
            g = grids[True][(w["peptides"][0], 0, False)]
            want = R.integrate(g, _st())
            assert g["matrix"].shape == (n * 3, 100) and g["ref"] == ref and want["peak"]
            assert want["warps"] == [s - shift[ref] for s in shift] and len(set(want["warps"])) == n
            assert len(set(want["areas"])) == n and min(want["areas"]) > 0.0
        return w, check
    return build


def _build_two_charges(db):
    w = draw(db, [dict(ref=0, traces={(2, False, 0): lobe(50), (2, False, 1): lobe(58, height=2.0 ** 19),
                                      (3, False, 0): lobe(50, height=2.0 ** 18), (3, False, 1): lobe(44, height=2.0 ** 21)}),
                  dict(ref=1, traces={(3, False, 0): lobe(45), (3, False, 1): lobe(50)})], 2)

    def check(w, grids):
        a, b = w["peptides"]
        assert sorted(grids[False]) == [(a, 2, False), (a, 3, False), (b, 3, False)] and sorted(grids[True]) == [(a, 0, False), (b, 0, False)]
        two, three = grids[False][(a, 2, False)], grids[False][(a, 3, False)]
        assert R.integrate(two, _st())["warps"] == [0, 8] and R.integrate(three, _st())["warps"] == [0, -6]
        both = grids[True][(a, 0, False)]["matrix"]
        assert np.allclose(both, two["matrix"] + three["matrix"], rtol=1e-12) and two["matrix"].any() and three["matrix"].any()
    return w, check


def _build_decoy(r):
    def build(db):
        c = 70  # (a clamped decoy's grid starts below 0: its bins under 50 cannot be drawn)
        ta, tb = lobe(c, 2.0, floor=2.0 ** -12), lobe(c + 4, 2.0, floor=2.0 ** -12)
        w = draw(db, [dict(ref=0, r=r, traces={(2, False, 0): ta, (2, True, 0): ta, (2, False, 1): tb, (2, True, 1): tb}),
                      dict(ref=0, r=0.5, traces={(2, False, 0): lobe(45, 2.0, 2.0 ** 22), (2, False, 1): lobe(45, 2.0, 2.0 ** 22)}),
                      dict(ref=0, r=0.7, traces={(2, False, 0): lobe(53, 2.0, 2.0 ** 21), (2, False, 1): lobe(52, 2.0, 2.0 ** 21)})], 2)

        def check(w, grids):
            a, b, c3 = w["peptides"]
            d = grids[True][(a, 0, True)]
            rd = max(w["art"][0] - R.RT_TOL * F32(2.0), F32(0.0))
            assert d["rt_min"] == rd - R.RT_TOL and (rd == 0.0) == (r is not None)
            st = _st("RetentionTime")
            res, passing, _ = R.quantify(st, CHARGES, None, None, None, 2, None, grids=grids[True])
            assert all(v["peak"] for v in res.values())
            assert res[(a, 0, False)]["score"] == res[(a, 0, True)]["score"] < res[(b, 0, False)]["score"], "the twins' scores are equal"
            # stable order of the f32 scores: b, c (1.0 each), target a, decoy a -> decoy / target = 1/1, 1/2, 1/3, 2/3; with the
            # decoy ahead of its twin it would be 1/1, 1/2, 2/2, 2/3
            third = F32(1.0) / F32(3.0)
            assert [res[k]["q_value"] for k in sorted(res)] == [third, F32(2.0) / F32(3.0), third, third]
        return w, check
    return build


_BUILDERS = {
    "silent_file": _build_silent_file,
    "silent_reference": _build_silent_reference,
    "large_shifts": _build_large_shifts,
    "tied_offsets": _build_tied_offsets,
    "reference_file_2": _build_reference_file_2,
    "plateau": _build_plateau,
    "grid_ends": _build_grid_ends,
    "equal_scores": _build_equal_scores,
    "threshold_stop": _build_threshold_stop,
    "threshold_fails": _build_threshold_fails,
    "proportional": _build_proportional(True),
    "proportional_below_one": _build_proportional(False),
    "one_file": _build_files(1, 0),
    "two_files": _build_files(2, 1),
    "nine_files": _build_files(9, 8),
    "two_charges": _build_two_charges,
    "decoy_twin": _build_decoy(None),
    "clamped_decoy": _build_decoy(0.004),
}
CASES = tuple(_BUILDERS)
_WORLDS = {}

# (case, scoring, threshold) whose decisions hang on the last bits of an angle: tests/test_lfq_integration_cpu.py finds them by
# nudging acos by ACOS_ULPS and requires this list to be exactly what it finds; on the device they are compared for matrix and
# warps only
FRAGILE = frozenset()


def case(db, name):
    """the named world, built and traced once: draw()'s dict plus grids = {combine: {key: grid}} of the restatement.  The
    case's defining property has been asserted on the restatement."""
    if name not in _WORLDS:
        w, check = _BUILDERS[name](db)
        combines = (True, False) if len(w["drawn_charges"]) > 1 else (True,)
        w["grids"] = {c: R.trace(w["fmap"], w["spectra"], w["alignments"], w["n_files"], c, isotopes_of(db)) for c in combines}
        assert 1 <= len(w["grids"][True]) and len(w["peptides"]) <= 6
        check(w, w["grids"])
        _WORLDS[name] = w
    return _WORLDS[name]


# ---- twelve small worlds: the parameters that have only ever had one value ------------------------------------------------------
N_WORLDS = 12
WORLD_FILES = (1, 2, 5, 9)
WORLD_CHARGES = ((1, 1), (2, 2), (3, 3), (1, 6), (2, 3), (4, 6))
WORLD_PPM = (1.0, 5.0, 20.0, 50.0)
WORLD_SEEDS = tuple(range(7000, 7000 + N_WORLDS))
_PARAM_WORLDS = {}


def ref_spectra_im(batches):
    import lfq_im_reference as RI
    out = []
    for b in batches:
        for i in range(b.n):
            lo, hi = int(b.peak_off[i]), int(b.peak_off[i + 1])
            if b.mobility is not None and b.has_mobility[i]:
                m, it, mob = RI.process_ms1(b.mz[lo:hi], b.intensities[lo:hi], b.mobility[lo:hi])
            else:
                (m, it), mob = R.process_ms1(b.mz[lo:hi], b.intensities[lo:hi]), None
            out.append((int(b.file_id[i]), F32(b.scan_start_time[i]), m, it, mob))
    return out


def _add_peaks(s, mz, intensity, mobility):
    """more peaks for a spectrum, every column through the same stable sort by m/z (equal m/z keep their order)"""
    allmz = np.concatenate([s.mz, np.asarray(mz, np.float32)])
    order = np.argsort(allmz, kind="stable")
    s.mz = allmz[order]
    s.intensity = np.concatenate([s.intensity, np.asarray(intensity, np.float32)])[order]
    if s.mobility is not None:
        s.mobility = np.concatenate([s.mobility, np.asarray(mobility, np.float32)])[order]


def param_settings(i):
    """what world i varies besides its spectra: (n_files, precursor_charge, combine, ppm, ion mobility, settings dict)"""
    n_files, charge = WORLD_FILES[i % 4], WORLD_CHARGES[i % 6]
    combine, ppm, im = bool((i // 2) % 2), WORLD_PPM[(i + i // 4) % 4], i % 2 == 1
    st = R.default_settings(peak_scoring=R.SCORING[(i + 3) % 4], integration=R.INTEGRATION[(i // 4) % 2],
                            spectral_angle=0.0 if i % 3 == 0 else 0.70, ppm_tolerance=ppm, combine_charge_states=combine)
    return n_files, charge, combine, ppm, im, st


def param_world(db, i):
    """World i of N_WORLDS from synthetic_lcms, its parameters drawn together (see param_settings), with alignments of slope in
    [0.8, 1.25], a non-zero intercept per file and max_rt != 1; the reference file mostly not file 0; one file split across two
    RawBatches, the batches out of file order, an empty RawBatch among them; spectra without peaks first, last and adjacent;
    duplicate m/z inside spectra; and -0.0, 0.0 and inf intensities in peaks that fall into a window.  (No NaN intensity: the
    sign and payload of a NaN are not fixed by IEEE arithmetic, the host's and the device's differ, and the grids are compared
    bit for bit.)  Built and traced by the restatement once; its conditions are asserted here."""
    if i in _PARAM_WORLDS:
        return _PARAM_WORLDS[i]
    import lfq_im_reference as RI
    from sage_amd.lcms import synthetic_ion_mobility
    n_files, charge, combine, ppm, im, settings = param_settings(i)
    seed = WORLD_SEEDS[i]
    rng = np.random.default_rng(seed)
    run = 60.0
    files = synthetic_lcms(db, n_files=n_files, n_peptides=int(rng.integers(8, 13)), ms1_per_file=int(rng.integers(60, 121)), seed=seed,
                           run_minutes=run, peak_width=0.02, ms1_noise=20, ms2_per_peptide=0, charges=tuple(range(charge[0], charge[1] + 1)))
    peps, apex = files[0].peptides, files[0].apex
    k0 = None
    if im:
        k0, mobility = synthetic_ion_mobility(db, files, seed=seed + 1, charges=tuple(range(charge[0], charge[1] + 1)))
        for f, lf in enumerate(files):
            for j, (s, m) in enumerate(zip(lf.spectra, mobility[f])):
                s.mobility = None if (f == 1 and j % 3 == 0) else m   # file 1: every third spectrum without the column
    max_rt = float(rng.uniform(400.0, 600.0))
    al = np.zeros(n_files, ALIGNMENT_DTYPE)
    for f in range(n_files):
        al[f] = (f, F32(max_rt), F32(rng.uniform(0.8, 1.25)), F32(-rng.uniform(0.01, 0.05)))
    # a file's own clock: the common coordinate u = apex-frame time / max_rt is what its alignment maps the scan start time to
    for f, lf in enumerate(files):
        for s in lf.spectra:
            u = (s.scan_start_time - lf.rt_shift) / lf.rt_scale / max_rt
            s.u = u
            s.scan_start_time = float(F32((u - float(al[f]["intercept"])) / float(al[f]["slope"]) * max_rt))
            assert s.scan_start_time >= 0.0
    rows = []
    for k, p in enumerate(peps):
        fid = n_files - 1 - (k % n_files)
        if fid == 0 and k % 4 == 1:
            fid = n_files - 1
        rows.append((int(p), 1, float(db.pep_mono[p]), fid, float(apex[k]) * run / max_rt + rng.normal(0.0, 0.0002), 0.0))
    f, art, pq = features_table(db, rows)
    assert n_files == 1 or (f["file_id"] != 0).sum() > len(f) // 2
    if im:
        f["ims"] = k0 * (1.0 + rng.uniform(-0.002, 0.002, len(k0))).astype(np.float32)
    # decoy windows with signal in the last file, so that the precursor FDR has decoys to count
    z0 = charge[0]
    for k in range(0, len(peps), 3):
        for s in files[-1].spectra:
            if abs(s.u - (float(art[k]) - 0.01)) < 0.004:
                bait = (float(db.pep_mono[peps[k]]) + np.arange(3) * 1.00335) / z0 + 11.06 + 1.0072764
                _add_peaks(s, bait, rng.lognormal(11.0, 1.0, 3), np.full(3, k0[k] if im else 0.0))
    # duplicate m/z: the five most intense peaks of every seventh spectrum once more (signal outweighs noise)
    for lf in files:
        for s in lf.spectra[::7]:
            top = np.argsort(s.intensity)[-5:]
            _add_peaks(s, s.mz[top], s.intensity[top] * F32(0.37), s.mobility[top] if s.mobility is not None else np.zeros(5))
    fmap_of = RI.build_feature_map if im else R.build_feature_map
    feats = dict(ref_feats(f, art, pq), **({"ims": f["ims"]} if im else {}))
    fmap = fmap_of(settings, charge, feats)
    # -0.0, 0.0 and inf in peaks that fall into a window: the first three spectra of the middle file that have such a peak
    special = [F32(np.inf), F32(-0.0), F32(0.0)]
    alignments = [tuple(a) for a in al.tolist()]
    for s in files[n_files // 2].spectra:
        if not special:
            break
        rt = R.spectrum_rt(F32(s.scan_start_time), alignments[n_files // 2])
        for j in np.argsort(s.intensity)[::-1][:8]:
            mass = F32(s.mz[j]) - R.PROTON
            hit = list(R.mass_lookup(fmap, rt, mass)) if s.mobility is None else list(RI.mass_mobility_lookup(fmap, rt, mass, F32(s.mobility[j])))
            if hit:
                s.intensity = s.intensity.copy()
                s.intensity[j] = special.pop(0)
                break
    assert not special, "every special intensity found a window"
    # spectra without peaks: first and two adjacent ones in file 0, last in the last file
    def empty(like, fid):
        return RawSpectrum(np.zeros(0, np.float32), np.zeros(0, np.float32), 0.0, None, None, like.scan_start_time, None, fid, "empty",
                           mobility=np.zeros(0, np.float32) if im else None)
    per_file = [list(lf.spectra) for lf in files]
    mid = len(per_file[0]) // 2
    per_file[0] = [empty(per_file[0][0], 0)] + per_file[0][:mid] + [empty(per_file[0][mid], 0), empty(per_file[0][mid], 0)] + per_file[0][mid:]
    per_file[-1] = per_file[-1] + [empty(per_file[-1][-1], n_files - 1)]
    # batches: file 0 split in two, the second half first; the other files in a drawn order; an empty batch among them
    whole = [RawBatch(sp) for sp in per_file]
    cut = whole[0].n // 2
    batches = [whole[0].slice(cut, whole[0].n)] + [whole[int(j)] for j in rng.permutation(np.arange(1, n_files))] + [whole[0].slice(0, cut)]
    batches.insert(1 + len(batches) // 2, RawBatch([]))
    assert sum(b.n for b in batches) == sum(len(sp) for sp in per_file)
    spectra = ref_spectra_im(batches) if im else ref_spectra(batches)
    grids = (RI.trace if im else R.trace)(fmap, spectra, alignments, n_files, combine, isotopes_of(db))
    ref, passing, _ = R.quantify(settings, charge, None, None, None, n_files, None, grids=grids)
    cc, ss = peptide_compositions(db.seq_off, db.seq)
    w = dict(f=f, art=art, pq=pq, al=al, batches=batches, carbon=cc, sulfur=ss, fmap=fmap, spectra=spectra, alignments=alignments,
             grids=grids, ref=ref, passing=passing, settings=settings, charge=charge, n_files=n_files, combine=combine, im=im, ppm=ppm)
    # the world's conditions
    assert len(grids) >= 6, len(grids)
    assert sum(r["peak"] for r in ref.values()) >= 3
    if charge[1] > charge[0] and not combine:
        assert len({k[1] for k in grids}) >= 2, "at least two charge states have a grid"
    cells = np.concatenate([g["matrix"].ravel() for g in grids.values()])
    assert np.isinf(cells).any() and not np.isnan(cells).any(), "the inf intensity reached a grid; no NaN (its bits are not portable)"
    assert not any(np.isnan(r["areas"]).any() for r in ref.values() if r["peak"])
    assert any(b.n == 0 for b in batches) and sum(1 for b in batches if b.n and (b.file_id == 0).all()) == 2
    _PARAM_WORLDS[i] = w
    return w
