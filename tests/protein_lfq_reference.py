"""Protein-level label-free quantification (MaxLFQ) restated in plain Python: loops over Python floats (IEEE f64,
one rounding per operation, no FMA), no numpy arithmetic in the numeric path.  Written from the contract's text, not from
sage_amd/csrc/maxlfq.h.  ln and exp are rounded correctly through `decimal` at 60 digits, the way tests/test_crlog.py holds cr_log.

    protein_lfq(areas, protein_of_row, n_proteins, min_ratio_count) -> dict of plain lists, one entry per protein
"""
import math
import struct
from decimal import Decimal, getcontext

NONE = 0xFFFFFFFF
NAN = float("nan")

_ln_cache = {}


def ln(x: float) -> float:
    """the correctly rounded natural logarithm of a positive finite double"""
    v = _ln_cache.get(x)
    if v is None:
        getcontext().prec = 60
        v = _ln_cache[x] = float(Decimal(x).ln())  # (Decimal(float) is exact; Decimal.ln and float() round correctly)
    return v


def exp(x: float) -> float:
    """the correctly rounded e^x of a finite double (overflow: inf; below the subnormals: 0.0)"""
    if x > 709.782712893384:
        return math.inf
    if x < -745.1332191019412:
        return 0.0
    getcontext().prec = 60
    return float(Decimal(x).exp())


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def ulp_distance(a: float, b: float) -> int:
    """the number of doubles between two finite doubles of the same sign (0: the same bits)"""
    return abs(bits(a) - bits(b))


def log_of_area(a: float) -> float:
    return ln(a) if (a > 0.0 and a < math.inf) else NAN


def pair_list(n_files: int):
    return [(j, k) for j in range(n_files) for k in range(j + 1, n_files)]


def median(values):
    s = sorted(values)
    c = len(s)
    return s[c // 2] if c % 2 else (s[c // 2 - 1] + s[c // 2]) * 0.5


def one_protein(L, n_files: int, min_ratio_count: int):
    """L: the protein's rows in ascending row index, each a list of n_files logs (NaN = missing).  Returns (pair_median, pair_count,
    component, log_abundance, n_components)."""
    need = max(int(min_ratio_count), 1)
    pairs = pair_list(n_files)
    # 2. pair medians
    med, cnt, valid = [], [], {}
    for (j, k) in pairs:
        d = [row[j] - row[k] for row in L if row[j] == row[j] and row[k] == row[k]]
        cnt.append(len(d))
        if len(d) >= need:
            m = median(d)
            med.append(m)
            valid[(j, k)] = m
        else:
            med.append(NAN)
    # 3. components; the label is the smallest file index
    label = list(range(n_files))
    for (j, k) in sorted(valid):  # ascending pairs: union by relabelling
        a, b = label[j], label[k]
        if a != b:
            lo, hi = min(a, b), max(a, b)
            label = [lo if x == hi else x for x in label]
    # 4. normal equations
    A = [[0.0] * n_files for _ in range(n_files)]
    b = [0.0] * n_files
    for (j, k) in valid:
        A[j][j] += 1.0
        A[k][k] += 1.0
        A[j][k] -= 1.0
        A[k][j] -= 1.0
    for j in range(n_files):
        s = 0.0
        for k in range(n_files):
            if j < k and (j, k) in valid:
                s = s + valid[(j, k)]
            elif k < j and (k, j) in valid:
                s = s - valid[(k, j)]
        b[j] = s
    for g in range(n_files):
        if label[g] == g:  # grounded
            for c in range(n_files):
                A[g][c] = 0.0
                A[c][g] = 0.0
            A[g][g] = 1.0
            b[g] = 0.0
    # 5. forward elimination without pivoting, back substitution
    for p in range(n_files):
        if A[p][p] == 0.0 or not math.isfinite(A[p][p]):
            raise ArithmeticError(f"pivot {p} is {A[p][p]}")
        for i in range(p + 1, n_files):
            if A[i][p] == 0.0:
                continue
            f = A[i][p] / A[p][p]
            for c in range(p, n_files):
                A[i][c] = A[i][c] - f * A[p][c]
            b[i] = b[i] - f * b[p]
    x = [0.0] * n_files
    for i in range(n_files - 1, -1, -1):
        s = b[i]
        for c in range(i + 1, n_files):
            s = s - A[i][c] * x[c]
        x[i] = s / A[i][i]
    # 6. anchor
    col, num = [0.0] * n_files, [0] * n_files
    for j in range(n_files):
        s = 0.0
        for row in L:
            if row[j] == row[j]:
                s = s + row[j]
                num[j] += 1
        col[j] = s
    out, comp, n_components = [NAN] * n_files, [NONE] * n_files, 0
    for g in range(n_files):
        if label[g] != g:
            continue
        members = [j for j in range(n_files) if label[j] == g]
        T, N, S = 0.0, 0, 0.0
        for j in members:
            T = T + col[j]
            N += num[j]
            S = S + x[j]
        if N == 0:
            continue
        n_components += 1
        shift = T / N - S / len(members)
        for j in members:
            out[j] = x[j] + shift
            comp[j] = g
    return med, cnt, comp, out, n_components


def protein_lfq(areas, protein_of_row, n_proteins: int, min_ratio_count: int = 1, n_files=None):
    """areas: n_rows lists of n_files floats; protein_of_row: n_rows ids (NONE: ignored).  Per protein: pair_median, pair_count,
    component, log_abundance, n_rows_used, n_components, intensity (the correctly rounded exp; 0.0 where not quantified)."""
    rows_of = [[] for _ in range(n_proteins)]
    for r, p in enumerate(protein_of_row):
        if int(p) != NONE:
            rows_of[int(p)].append(r)
    if n_files is None:
        n_files = len(areas[0]) if len(areas) else 0
    res = dict(pair_median=[], pair_count=[], component=[], log_abundance=[], n_rows_used=[], n_components=[], intensity=[])
    for p in range(n_proteins):
        L = [[log_of_area(float(a)) for a in areas[r]] for r in rows_of[p]]
        med, cnt, comp, la, nc = one_protein(L, n_files, min_ratio_count)
        res["pair_median"].append(med)
        res["pair_count"].append(cnt)
        res["component"].append(comp)
        res["log_abundance"].append(la)
        res["n_rows_used"].append(len(L))
        res["n_components"].append(nc)
        res["intensity"].append([exp(v) if v == v else 0.0 for v in la])
    return res
