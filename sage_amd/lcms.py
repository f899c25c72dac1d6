"""Synthetic multi-file LC-MS runs (MS1 + MS2) for label-free quantification, and SPS-MS3 runs for TMT quantification.

Each file holds the same peptides eluting as Gaussians in retention time; every file has its own RT scale and shift.  MS1
scans carry the peptides' Poisson isotope envelopes at charges 2..4 plus uniform noise centroids; MS2 scans near each
peptide's apex use the b/y model of synthetic.synthetic_spectra, so the search identifies them.  All randomness comes from
numpy.random.default_rng(seed).
"""
import os
from dataclasses import dataclass
from typing import List

import numpy as np

from .api import IndexedDatabase, RawSpectrum
from .synthetic import _MASS_LUT, PROTON

NEUTRON = 1.00335


@dataclass
class LcmsFile:
    spectra: List[RawSpectrum]  # in scan order (scan start time ascending)
    ms_levels: List[int]
    rt_scale: float
    rt_shift: float
    peptides: np.ndarray        # the peptides of the experiment
    apex: np.ndarray            # their apex, as a fraction of the run (before the file's scale and shift)


def _ms2(db: IndexedDatabase, pep: int, z: int, rng, noise_peaks: int, keep_prob: float, ppm_sigma: float):
    a, b = int(db.seq_off[pep]), int(db.seq_off[pep + 1])
    res = _MASS_LUT[db.seq[a:b]] + db.mods[a:b].astype(np.float64)
    nterm = float(db.nterm[pep]) if not np.isnan(db.nterm[pep]) else 0.0
    mono = float(db.pep_mono[pep])
    bs = nterm + np.cumsum(res)[:-1]
    frag = np.concatenate([bs, mono - bs])
    cand = [frag + PROTON] + ([(frag + 2 * PROTON) / 2.0] if z >= 3 else [])
    cand = np.concatenate(cand)
    keep = rng.random(len(cand)) < keep_prob
    mz = np.concatenate([cand[keep] * (1.0 + rng.normal(0.0, ppm_sigma, keep.sum()) * 1e-6), rng.uniform(150.0, 1800.0, noise_peaks)])
    it = np.concatenate([rng.lognormal(8.0, 1.2, keep.sum()), rng.lognormal(6.5, 1.0, noise_peaks)])
    ok = (mz > 100.0) & (mz < 2500.0)
    order = np.argsort(mz[ok], kind="stable")
    prec = (mono + z * PROTON) / z * (1.0 + rng.normal(0.0, ppm_sigma) * 1e-6)
    return mz[ok][order].astype(np.float32), it[ok][order].astype(np.float32), prec


def poisson_envelope(mass: float, n: int = 4) -> np.ndarray:
    """relative isotope abundances ~ Poisson(mass / 1800)"""
    lam = mass / 1800.0
    k = np.arange(n)
    p = np.exp(-lam) * lam ** k / np.array([1, 1, 2, 6, 24, 120][:n])
    return p / p.max()


def synthetic_lcms(db: IndexedDatabase, n_files: int = 3, n_peptides: int = 40, ms1_per_file: int = 200, seed: int = 0,
                   run_minutes: float = 60.0, peak_width: float = 0.002, ms1_noise: int = 60, ms2_per_peptide: int = 2,
                   charges=(2, 3, 4), ppm_sigma: float = 2.0, ms2_noise: int = 40, keep_prob: float = 0.6,
                   peptides=None) -> List[LcmsFile]:
    """Files of one LC-MS experiment.  peak_width: Gaussian sigma of an elution profile, as a fraction of the run.  A file's
    retention time is `apex * rt_scale + rt_shift` (minutes).  peptides: target peptide indices (default: drawn)."""
    rng = np.random.default_rng(seed)
    targets = np.flatnonzero(db.decoy == 0)
    peps = np.asarray(peptides) if peptides is not None else rng.choice(targets, size=min(n_peptides, len(targets)), replace=False)
    apex = rng.uniform(0.12, 0.88, len(peps))               # fraction of the run
    abundance = rng.lognormal(13.0, 1.0, len(peps))
    zfrac = rng.dirichlet(np.ones(len(charges)), len(peps))  # charge-state distribution per peptide
    mono = db.pep_mono[peps].astype(np.float64)
    env = [poisson_envelope(m) for m in mono]
    files = []
    for f in range(n_files):
        scale = 1.0 + rng.uniform(-0.03, 0.03) if f else 1.0
        shift = rng.uniform(-0.01, 0.01) * run_minutes if f else 0.0
        times = (np.arange(ms1_per_file) + 0.5) / ms1_per_file * run_minutes
        entries = []  # (time, level, spectrum)
        sigma = peak_width * run_minutes
        centers = apex * run_minutes * scale + shift
        for t in times:
            mzs, ints = [rng.uniform(300.0, 1600.0, ms1_noise)], [rng.lognormal(7.0, 1.0, ms1_noise)]
            near = np.flatnonzero(np.abs(t - centers) < 4.0 * sigma)
            for p in near:
                h = abundance[p] * np.exp(-0.5 * ((t - centers[p]) / sigma) ** 2) * rng.lognormal(0.0, 0.05)
                for zi, z in enumerate(charges):
                    iso = np.arange(len(env[p]))
                    mz = (mono[p] + iso * NEUTRON) / z + PROTON
                    mzs.append(mz * (1.0 + rng.normal(0.0, ppm_sigma, len(mz)) * 1e-6))
                    ints.append(h * zfrac[p, zi] * env[p])
            mz = np.concatenate(mzs)
            it = np.concatenate(ints)
            order = np.argsort(mz, kind="stable")
            entries.append((t, 1, mz[order].astype(np.float32), it[order].astype(np.float32), 0.0, None))
        for p in range(len(peps)):
            for k in range(ms2_per_peptide):
                t = centers[p] + rng.normal(0.0, 0.3 * sigma)
                z = int(rng.choice(charges))
                mz, it, prec = _ms2(db, int(peps[p]), z, rng, ms2_noise, keep_prob, ppm_sigma)
                entries.append((t, 2, mz, it, prec, z))
        entries.sort(key=lambda e: e[0])
        spectra, levels = [], []
        for i, (t, lvl, mz, it, prec, z) in enumerate(entries):
            spectra.append(RawSpectrum(mz, it, float(np.float32(prec)), z, None, scan_start_time=float(np.float32(max(t, 0.0))),
                                       file_id=f, id=f"scan={i + 1}"))
            levels.append(lvl)
        files.append(LcmsFile(spectra, levels, scale, shift, peps, apex))
    return files


def write_lcms(directory: str, files: List[LcmsFile], stem: str = "run", mobility=None) -> List[str]:
    """mobility: per file, write_mzml's per-spectrum ion-mobility arrays (synthetic_ion_mobility), or None"""
    from .mzml import write_mzml
    os.makedirs(directory, exist_ok=True)
    paths = []
    for f, lf in enumerate(files):
        path = os.path.join(directory, f"{stem}{f}.mzML")
        if mobility is None or mobility[f] is None:
            write_mzml(path, lf.spectra, lf.ms_levels)
        else:
            write_mzml(path, lf.spectra, lf.ms_levels, mobility=mobility[f])
        paths.append(path)
    return paths


def synthetic_ion_mobility(db: IndexedDatabase, files: List[LcmsFile], seed: int = 0, spread_pct: float = 1.5, ppm: float = 15.0,
                           charges=(2, 3, 4), n_isotopes: int = 4):
    """An ion-mobility dimension for synthetic_lcms files.  Every peptide of the experiment gets a mobility k0 in [0.6, 1.4].
    An MS2 spectrum of the peptide (found by its precursor m/z and charge) gets inverse_ion_mobility = k0, in place — the search
    copies it to Feature.ims.  An MS1 peak within `ppm` of one of the peptide's charge x isotope m/z gets k0 * (1 + u / 100), u
    uniform in +-spread_pct, so a mobility window narrower than the spread keeps some of a peptide's peaks and drops others; every
    other peak gets a uniform mobility in [0.5, 1.6].  Returns (k0 per peptide, per file the per-spectrum f32 arrays — None for
    spectra above level 1 —, the shape write_lcms / write_mzml take)."""
    rng = np.random.default_rng(seed)
    peps = files[0].peptides
    k0 = rng.uniform(0.6, 1.4, len(peps)).astype(np.float32)
    mono = db.pep_mono[peps].astype(np.float64)
    z = np.asarray(charges, dtype=np.float64)
    table = ((mono[:, None, None] + np.arange(n_isotopes)[None, None, :] * NEUTRON) / z[None, :, None] + PROTON).reshape(-1)
    owner = np.repeat(np.arange(len(peps)), len(charges) * n_isotopes)
    order = np.argsort(table)
    table, owner = table[order], owner[order]
    out = []
    for lf in files:
        per_spectrum = []
        for s, lvl in zip(lf.spectra, lf.ms_levels):
            if lvl != 1:
                if s.precursor_charge:
                    m = (s.precursor_mz - PROTON) * s.precursor_charge
                    p = int(np.argmin(np.abs(mono - m)))
                    if abs(mono[p] - m) <= 50e-6 * m:
                        s.inverse_ion_mobility = float(k0[p])
                per_spectrum.append(None)
                continue
            mz = s.mz.astype(np.float64)
            mob = rng.uniform(0.5, 1.6, len(mz))
            j = np.clip(np.searchsorted(table, mz), 1, len(table) - 1)
            j = np.where(np.abs(table[j - 1] - mz) < np.abs(table[j] - mz), j - 1, j)
            hit = np.abs(table[j] - mz) <= ppm * 1e-6 * mz
            mob[hit] = k0[owner[j[hit]]] * (1.0 + rng.uniform(-spread_pct, spread_pct, int(hit.sum())) / 100.0)
            per_spectrum.append(mob.astype(np.float32))
        out.append(per_spectrum)
    return k0, out


@dataclass
class SpsFile:
    spectra: List[RawSpectrum]  # in scan order: MS1, then per precursor an MS2 and its MS3
    ms_levels: List[int]
    noise: list                 # per spectrum: noise array or None
    extra_precursors: list      # per spectrum: further SPS precursor m/z or None


def synthetic_sps_ms3(db: IndexedDatabase, labels, n_files: int = 2, ms2_per_file: int = 60, seed: int = 0, ms1_every: int = 10,
                      ms3_noise: int = 30, ms2_noise: int = 40, reporter_ppm: float = 4.0, noise_prob: float = 0.8,
                      run_minutes: float = 30.0) -> List[SpsFile]:
    """SPS-MS3 runs: every MS2 (b/y model of _ms2, searchable) is followed by an MS3 whose precursors are several of the MS2's
    fragments (spectrumRef = the MS2's id).  The MS3 holds a cluster of reporter peaks near `labels` (some labels missing, some
    with a close neighbour inside +-20 ppm), random noise peaks and, with probability noise_prob, a noise array (MS:1002744);
    every MSn spectrum has an ion injection time.  An MS1 scan every ms1_every precursors.  All randomness: default_rng(seed)."""
    rng = np.random.default_rng(seed)
    labels = np.asarray(labels, dtype=np.float64)
    targets = np.flatnonzero(db.decoy == 0)
    files = []
    for f in range(n_files):
        spectra, levels, noise, extra = [], [], [], []
        t = 0.0
        peps = rng.choice(targets, size=ms2_per_file, replace=len(targets) < ms2_per_file)
        for k, pep in enumerate(peps):
            if k % ms1_every == 0:
                mz = np.sort(rng.uniform(350.0, 1500.0, 50)).astype(np.float32)
                spectra.append(RawSpectrum(mz, rng.lognormal(8.0, 1.0, 50).astype(np.float32), 0.0, None,
                                           scan_start_time=float(np.float32(t)), file_id=f, id=f"scan={len(spectra) + 1}"))
                levels.append(1), noise.append(None), extra.append(None)
            t += run_minutes / (ms2_per_file * 2.2)
            z = int(rng.choice([2, 3]))
            mz, it, prec = _ms2(db, int(pep), z, rng, ms2_noise, 0.6, 2.0)
            ms2_id = f"controllerType=0 controllerNumber=1 scan={len(spectra) + 1}"
            iit2 = float(np.float32(rng.uniform(5.0, 50.0)))
            spectra.append(RawSpectrum(mz, it, float(np.float32(prec)), z, None, scan_start_time=float(np.float32(t)), file_id=f,
                                       id=ms2_id, ion_injection_time=iit2))
            levels.append(2), noise.append(None), extra.append(None)
            # the MS3: reporters (+ near neighbours) and noise, m/z ascending
            present = rng.random(len(labels)) < 0.9
            rep = labels[present] * (1.0 + rng.normal(0.0, reporter_ppm, present.sum()) * 1e-6)
            near = labels[rng.random(len(labels)) < 0.2] * (1.0 + rng.uniform(-15.0, 15.0) * 1e-6)
            rmz = np.concatenate([rep, near, rng.uniform(100.0, 1200.0, ms3_noise)])
            rit = np.concatenate([rng.lognormal(9.0, 1.0, len(rep)), rng.lognormal(6.0, 1.0, len(near)),
                                  rng.lognormal(6.5, 1.0, ms3_noise)])
            o = np.argsort(rmz, kind="stable")
            rmz, rit = rmz[o].astype(np.float32), rit[o].astype(np.float32)
            sps = mz[rng.choice(len(mz), size=min(len(mz), 5), replace=False)] if len(mz) else np.zeros(0, np.float32)
            spectra.append(RawSpectrum(rmz, rit, float(sps[0]) if len(sps) else float(np.float32(prec)), None, None,
                                       scan_start_time=float(np.float32(t)), file_id=f, id=f"scan={len(spectra) + 1}",
                                       ion_injection_time=float(np.float32(rng.uniform(20.0, 120.0))), precursor_ref=ms2_id))
            levels.append(3)
            noise.append(rng.uniform(50.0, 500.0, len(rmz)).astype(np.float32) if rng.random() < noise_prob else None)
            extra.append([float(x) for x in sps[1:]])
        files.append(SpsFile(spectra, levels, noise, extra))
    return files


def write_sps(directory: str, files: List[SpsFile], stem: str = "sps") -> List[str]:
    from .mzml import write_mzml
    os.makedirs(directory, exist_ok=True)
    paths = []
    for f, sf in enumerate(files):
        path = os.path.join(directory, f"{stem}{f}.mzML")
        write_mzml(path, sf.spectra, sf.ms_levels, sf.noise, sf.extra_precursors)
        paths.append(path)
    return paths
