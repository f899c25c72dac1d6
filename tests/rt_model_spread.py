"""How far the predictions of the retention / mobility models move when nothing but the order of the sums and the last bits
of ln_1p change — measured with the oracle alone (never with the device), per world, and kept in profiles/rt_model_spread.json.

The normal equations are rank deficient and solved through a 1e-8 regulariser, so that legitimate noise is amplified by an
amount that depends on the world (2e-12 on 20 000 rows, 3e-6 on the mobility model of 500).  measure() refits the oracle
(oracle_lib.linreg_fit on the oracle's own embedded rows) REFITS times with the training rows permuted and, for the retention
model, the ln_1p column moved by up to 2 ulps per row, and returns the largest difference between any two of the refits'
predictions.  tests/test_gpu_rescore.py: rt_tolerance() turns that into compare_rt()'s bound; the device's blocked order and its
libm are one more draw from the same family.

    python tests/rt_model_spread.py        rewrites profiles/rt_model_spread.json (tests/test_rt_model_cpu.py recomputes two
                                           entries and holds them to the file within a factor of 4)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "profiles", "rt_model_spread.json")
REFITS = 16
LN1P_COLUMN = 22 * 3 + 1  # retention_model.rs:36 PEPTIDE_MASS


def _predictions(rows, beta, hi):
    pred = np.zeros(len(rows))
    for j in range(rows.shape[1]):
        pred = pred + rows[:, j] * beta[j]
    return np.clip(pred, 0.0, hi)


def measure(f, n_files, seq_off, seq, mono, seed=1):
    """{"rt": spread, "ims": spread, "n": rows, "train": training rows}.  A spread is 0.0 where the model is not fitted or predicts
    no finite number, inf where a refit decides differently from the others whether the model is fitted at all."""
    import oracle_lib
    o = oracle_lib.predict_rt(f, n_files, seq_off, seq, mono)
    train = (f["label"] == 1) & (o["spectrum_q"] <= np.float32(0.01))
    out = dict(n=int(len(f)), train=int(train.sum()))
    rng = np.random.default_rng(seed)
    t = np.flatnonzero(train)
    for key, rows, y, hi in (("rt", oracle_lib.embed_rows(seq_off, seq, mono), o["aligned_rt"].astype(np.float64), 1.0),
                             ("ims", oracle_lib.embed_rows(seq_off, seq, mono, f["charge"]), f["ims"].astype(np.float64), 2.0)):
        lo_p = hi_p = None
        fitted = set()
        for r in range(REFITS if len(t) else 0):
            x = rows
            if key == "rt":  # up to 2 ulps on ln_1p(mono), in the fit and in the prediction alike (one libm serves both)
                x = rows.copy()
                col = x[:, LN1P_COLUMN]
                x[:, LN1P_COLUMN] = col + rng.integers(-2, 3, len(col)) * np.spacing(col)
            order = rng.permutation(t)
            fit = oracle_lib.linreg_fit(x[order], y[order])
            fitted.add(fit is not None)
            if fit is None:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                p = _predictions(x, fit[0], hi)
            lo_p = p if lo_p is None else np.fmin(lo_p, p)
            hi_p = p if hi_p is None else np.fmax(hi_p, p)
        if len(fitted) == 2:
            out[key] = float("inf")
        elif lo_p is None:
            out[key] = 0.0
        else:
            d = (hi_p - lo_p)[np.isfinite(hi_p - lo_p)]
            out[key] = float(d.max()) if len(d) else 0.0
    return out


def cases():
    """name -> (features, n_files, seq_off, seq, mono): the worlds of test_predict_rt_synthetic, test_predict_rt_degenerate_inputs
    and test_predict_rt_edge_case.  (test_search_predict_rescore_chain's features come out of the device search: measured there.)"""
    from rescore_edge_cases import RT_CASES
    from sage_amd.synthetic import synthetic_rt_world
    c = {}
    for n, n_files, seed in SYNTHETIC:
        f, off, seq, mono = synthetic_rt_world(n, n_files, seed=seed)
        c[synthetic_name(n, n_files, seed)] = (f, n_files, off, seq, mono)
    f, off, seq, mono = synthetic_rt_world(4000, 2, seed=12, with_ims=False)
    c["degenerate/no_ims"] = (f, 2, off, seq, mono)
    f0 = f.copy()
    f0["label"] = -1
    c["degenerate/no_targets"] = (f0, 2, off, seq, mono)
    c.update(RT_CASES)
    return c


SYNTHETIC = [(20000, 3, 9), (500, 1, 10), (60000, 8, 11)]


def synthetic_name(n, n_files, seed):
    return f"synthetic/n{n}_f{n_files}_s{seed}"


def load():
    with open(PATH) as fh:
        return json.load(fh)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    table = {}
    for name, case in cases().items():
        with np.errstate(invalid="ignore", divide="ignore"):
            table[name] = measure(*case)
        print(name, table[name], flush=True)
    with open(PATH, "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")
