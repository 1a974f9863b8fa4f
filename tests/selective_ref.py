"""The numpy fp64 restatement of ``slnlp_selective_rows`` / ``_counts`` (include/slnlp.h): per row the arg-max, the code, whether the
arg-max is wrong, the confidence and whether a threshold accepts it; per included row the number of rows (and of wrong rows) at
least as confident; the summary table and the report.  Test infrastructure only.

z float32 log-probs [N, V], beta a number.  zmax the row maximum, a = beta zmax, e_c = exp(beta z_c - a) over the columns NOT at
the maximum, n_max the columns at it, rest = sum e + (n_max - 1), s0 = 1 + rest.  Codes: -2 a NaN or a maximum that is not finite
(first), -1 a label outside [0, V), else 0.  kappa: 1 / s0 (max_prob); 0 for n_max >= 2 else (1 - max e) / s0 (margin); (sum e t) / s0 -
log1p(rest) with t = beta z - a and 0 for a term with e == 0 (neg_entropy).  Included: code 0 and kappa no NaN.  ge_i / ge_wrong_i
count the included (wrong) rows with kappa_j >= kappa_i; -0.0 equals +0.0.  AURC = (1 / n) sum ge_wrong_i / ge_i, added with
``math.fsum``."""
import math

import numpy as np

SCORES = ("max_prob", "margin", "neg_entropy")
HEAD, LEVELS, CHUNK = 40, 8, 2048          # SLNLP_SEL_TABLE_HEAD, SLNLP_SEL_MAX_LEVELS, SLNLP_SEL_CHUNK


def rows_ref(z, y=None, beta=1.0, score="max_prob", tau=None):
    """{kappa float64 [N] (NaN for code -2), rows int64 [N, 4] = (pred, wrong, accepted, code)}."""
    z = np.asarray(z, dtype=np.float32)
    zz = z.astype(np.float64)
    N, V = zz.shape
    with np.errstate(all="ignore"):
        pred = np.argmax(z, axis=1)                          # a NaN first, then the first maximum
        zmax = zz.max(axis=1)
        bad = ~np.isfinite(zmax) | np.isnan(zz).any(axis=1)
        at_max = zz == zmax[:, None]
        t = beta * zz - (beta * zmax)[:, None]
        e = np.where(at_max, 0.0, np.exp(t))
        n_max = at_max.sum(axis=1)
        rest = e.sum(axis=1) + (n_max - 1.0)
        s0 = 1.0 + rest
        if score == "max_prob":
            kappa = 1.0 / s0
        elif score == "margin":
            kappa = np.where(n_max >= 2, 0.0, (1.0 - e.max(axis=1)) / s0)
        elif score == "neg_entropy":
            et = np.where(e != 0.0, e * np.where(e != 0.0, t, 0.0), 0.0)
            kappa = np.array([math.fsum(r) for r in et]) / s0 - np.log1p(rest)
        else:
            raise ValueError(score)
    kappa = np.where(bad, np.nan, kappa)
    rows = np.zeros((N, 4), dtype=np.int64)
    rows[:, 0] = pred
    rows[bad, 3] = -2
    if y is not None:
        y = np.asarray(y).astype(np.int64)
        inside = (y >= 0) & (y < V)
        rows[~bad & ~inside, 3] = -1
        rows[:, 1] = (rows[:, 3] == 0) & (pred != y)
    if tau is not None:
        with np.errstate(invalid="ignore"):
            rows[:, 2] = kappa >= tau                        # a NaN: rejected
    return {"kappa": kappa, "rows": rows}


def included(kappa, rows):
    return (np.asarray(rows)[:, 3] == 0) & ~np.isnan(np.asarray(kappa, dtype=np.float64))


def counts_ref(kappa, rows):
    """int64 [N, 2]: (ge, ge_wrong) per included row, (0, 0) for the others."""
    kappa, rows = np.asarray(kappa, dtype=np.float64), np.asarray(rows)
    inc = included(kappa, rows)
    k = kappa[inc] + 0.0                                     # -0.0 + 0.0 = +0.0
    wrong = rows[inc, 1] != 0
    ks, kw = np.sort(k), np.sort(k[wrong])
    counts = np.zeros((len(kappa), 2), dtype=np.int64)
    counts[inc, 0] = ks.size - np.searchsorted(ks, k, side="left")
    counts[inc, 1] = kw.size - np.searchsorted(kw, k, side="left")
    return counts


def aurc_oracle(n, E):
    return math.fsum((k - n + E) / k for k in range(n - E + 1, n + 1)) / n if n else float("nan")


def summary_ref(kappa, rows, risks=(), coverages=()):
    """What the table says, from ``counts_ref``: {n, E, excluded_labels, excluded_nan, risk_sum, aurc, at_risk [(ge, ge_wrong)],
    at_coverage [(ge, ge_wrong)], counts}."""
    kappa, rows = np.asarray(kappa, dtype=np.float64), np.asarray(rows)
    counts = counts_ref(kappa, rows)
    inc = included(kappa, rows)
    ge, gw = counts[inc, 0], counts[inc, 1]
    n = int(inc.sum())
    S = math.fsum(float(w) / float(g) for g, w in zip(ge, gw))
    at_risk, at_cov = [], []
    for r in risks:
        ok = gw.astype(np.float64) <= float(r) * ge.astype(np.float64)
        i = np.flatnonzero(ok)[np.argmax(ge[ok])] if ok.any() else None
        at_risk.append((0, 0) if i is None else (int(ge[i]), int(gw[i])))
    for c in coverages:
        ok = ge.astype(np.float64) >= np.ceil(float(c) * float(n))
        i = np.flatnonzero(ok)[np.argmin(ge[ok])] if ok.any() else None
        at_cov.append((0, 0) if i is None else (int(ge[i]), int(gw[i])))
    return {"n": n, "E": int((rows[inc, 1] != 0).sum()), "excluded_labels": int((~inc & (rows[:, 3] == -1)).sum()),
            "excluded_nan": int((~inc & (rows[:, 3] != -1)).sum()), "risk_sum": S, "aurc": S / n if n else float("nan"),
            "at_risk": at_risk, "at_coverage": at_cov, "counts": counts}


def table_ref(kappa, rows, risks=(), coverages=()):
    """The table as the device lays it out (the chunk sums by ``math.fsum`` over each chunk of included rows in row order)."""
    s = summary_ref(kappa, rows, risks, coverages)
    N = len(kappa)
    table = np.zeros(HEAD + (N + CHUNK - 1) // CHUNK)
    table[:6] = [s["n"], s["E"], s["excluded_labels"], s["excluded_nan"], s["risk_sum"], s["aurc"]]
    for l, (g, w) in enumerate(s["at_risk"]):
        table[8 + 2 * l:10 + 2 * l] = g, w
    for l, (g, w) in enumerate(s["at_coverage"]):
        table[8 + 2 * LEVELS + 2 * l:10 + 2 * LEVELS + 2 * l] = g, w
    inc = np.flatnonzero(included(kappa, rows))
    for b in range(0, len(inc), CHUNK):
        c = s["counts"][inc[b:b + CHUNK]]
        table[HEAD + b // CHUNK] = math.fsum(float(w) / float(g) for g, w in c)
    return table, s


def curve_ref(kappa, rows):
    """The distinct thresholds in descending order: {threshold, accepted, wrong, coverage, risk}, by brute force."""
    kappa, rows = np.asarray(kappa, dtype=np.float64), np.asarray(rows)
    inc = included(kappa, rows)
    k, wrong = kappa[inc] + 0.0, rows[inc, 1] != 0
    thr = np.unique(k)[::-1]
    acc = np.array([(k >= t).sum() for t in thr], dtype=np.int64)
    wr = np.array([(wrong & (k >= t)).sum() for t in thr], dtype=np.int64)
    return {"threshold": thr, "accepted": acc, "wrong": wr, "coverage": acc / max(1, k.size), "risk": wr / np.maximum(acc, 1)}


def make_counts_case(N, seed, levels=None, error_rate=0.3, excluded=0.0, signed=False):
    """(kappa float64 [N], rows int32 [N, 4]) fed to the counts kernel directly: ``levels`` quantises kappa (ties), ``excluded`` is
    the share of rows with code -1 / -2 (a -2 row's kappa is a NaN), ``signed`` centres kappa on 0."""
    rs = np.random.RandomState(seed)
    kappa = rs.rand(N) if levels is None else rs.randint(0, levels, size=N) / float(levels)
    if signed:
        kappa = kappa - 0.5
    rows = np.zeros((N, 4), dtype=np.int32)
    rows[:, 0] = rs.randint(0, 7, size=N)
    rows[:, 1] = rs.rand(N) < error_rate
    code = np.where(rs.rand(N) < excluded, rs.choice([-1, -2], size=N), 0)
    rows[:, 3] = code
    rows[code != 0, 1] = 0
    kappa[code == -2] = np.nan
    return kappa, rows
