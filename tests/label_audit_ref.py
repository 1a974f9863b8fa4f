"""The numpy fp64 restatement of ``slnlp_label_audit`` and ``slnlp_scatter_logp`` (include/slnlp.h): the confident-learning audit of
a set of labelled log-probs (Northcutt, Jiang and Chuang 2021).  Test infrastructure only.

z float32 log-probs [N, V], y int64 [N], beta a number.  zmax the row maximum, a = beta zmax, e_c = exp(beta z_c - a) over the
columns NOT at the maximum, n_max the columns at it, rest = sum e + (n_max - 1), s0 = 1 + rest.  The probability of a column is
1 / s0 at the maximum and e_c / s0 elsewhere.  Codes: -2 a NaN or a maximum that is not finite (first), -1 a label outside [0, V),
else 0; only code 0 is usable.  s = p of the label, other = p of the first column other than the label in the arg-max's order
(larger float32 value first, equal values by ascending column; 0 for V = 1), m = s - other.  t_c = fsum(s over the usable rows
labelled c) / n_c, NaN for n_c = 0.  k = the first column with p >= t_c in that order, -1 for none.  flags: bit 0 k >= 0 and k != y,
bit 1 pred != y.  joint[y][k] counts the usable rows with k >= 0, every other row goes to the overflow cell."""
import math

import numpy as np


def audit_ref(z, y, beta=1.0, pairs=20):
    z = np.asarray(z, dtype=np.float32)
    y = np.asarray(y).astype(np.int64)
    zz = z.astype(np.float64)
    N, V = zz.shape
    with np.errstate(all="ignore"):
        pred = np.argmax(z, axis=1)                          # a NaN first, then the first maximum
        zmax = zz.max(axis=1)
        bad = ~np.isfinite(zmax) | np.isnan(zz).any(axis=1)
        at_max = zz == zmax[:, None]
        e = np.where(at_max, 0.0, np.exp(beta * zz - (beta * zmax)[:, None]))
        rest = e.sum(axis=1) + (at_max.sum(axis=1) - 1.0)
        s0 = 1.0 + rest
        P = np.where(at_max, (1.0 / s0)[:, None], e / s0[:, None])
    code = np.where(bad, -2, np.where((y < 0) | (y >= V), -1, 0)).astype(np.int64)
    usable = code == 0
    order = np.zeros((N, V), dtype=np.int64)
    order[usable] = np.argsort(-z[usable], axis=1, kind="stable")               # larger first, equal values by ascending column
    place = np.empty((N, V), dtype=np.int64)                                     # place[i, c]: where column c stands in row i's order
    np.put_along_axis(place, order, np.broadcast_to(np.arange(V), (N, V)), axis=1)

    def first(members):
        """Per row the first column of ``members`` (bool [N, V]) in the row's order, -1 for none."""
        at = np.where(members, place, V)
        return np.where(at.min(axis=1) < V, at.argmin(axis=1), -1)
    nan = float("nan")
    rows, label = np.arange(N), np.where(usable, y, 0)
    s = np.where(usable, P[rows, label], nan)
    runner = first(np.arange(V)[None, :] != label[:, None])                      # the first column other than the label (V = 1: none)
    other = np.where(usable, np.where(runner >= 0, P[rows, np.maximum(runner, 0)], 0.0), nan)
    m = s - other
    p_pred = np.where(bad, nan, 1.0 / s0)
    n = np.array([int((usable & (y == c)).sum()) for c in range(V)], dtype=np.int64)
    t = np.array([math.fsum(s[usable & (y == c)]) / n[c] if n[c] else nan for c in range(V)])
    with np.errstate(invalid="ignore"):
        K = P >= t[None, :]                                  # a NaN threshold compares false
    k = np.where(usable, first(K), -1)
    flags = np.where(usable, ((k >= 0) & (k != y)).astype(np.int64) | ((pred != y).astype(np.int64) << 1), 0)
    joint = np.zeros((V, V), dtype=np.int64)
    counted = usable & (k >= 0)
    np.add.at(joint, (y[counted], k[counted]), 1)
    cells = [(-int(joint[g, c]), g * V + c) for g in range(V) for c in range(V) if g != c and joint[g, c] > 0]
    top = [(f // V, f % V, -cnt) for cnt, f in sorted(cells)[:pairs]]
    return {"pred": pred, "code": code, "s": s, "other": other, "m": m, "p_pred": p_pred, "n": n, "t": t, "k": k, "flags": flags,
            "joint": joint, "overflow": int(N - counted.sum()), "pairs": top, "P": P,
            "counts": {"usable": int(usable.sum()), "bad_labels": int((code == -1).sum()), "nan_rows": int((code == -2).sum()),
                       "unconfident": int((usable & (k < 0)).sum()), "issues": int((flags & 1).sum()),
                       "argmax_disagrees": int(((flags >> 1) & 1).sum())}}


def smallest_gap(ref, y):
    """The least |p_ic - t_c| over the usable rows and the classes with a threshold, leaving out the (row, own class) pair of a
    single-row class, where equality is exact by the definition (inf when nothing is left)."""
    y = np.asarray(y).astype(np.int64)
    usable = ref["code"] == 0
    with np.errstate(invalid="ignore"):
        gap = np.abs(ref["P"] - ref["t"][None, :])
    gap[~usable] = np.inf
    gap[:, np.isnan(ref["t"])] = np.inf
    for i in np.flatnonzero(usable):
        if ref["n"][y[i]] == 1:
            assert ref["P"][i, y[i]] == ref["t"][y[i]]       # exact: fsum of one term, divided by 1
            gap[i, y[i]] = np.inf
    return float(gap.min()) if gap.size else float("inf")


def record_of(ref):
    """The restatement as ``ops.label_audit_download``'s dict, for ``metrics.label_audit_report``."""
    return {"head": np.array([ref["counts"][q] for q in ("usable", "bad_labels", "nan_rows", "unconfident", "issues", "argmax_disagrees")]
                             + [0, 0], dtype=np.int64),
            "t": ref["t"], "n": ref["n"].astype(np.int32), "joint": ref["joint"], "overflow": ref["overflow"],
            "pairs": np.array([list(p) for p in ref["pairs"]], dtype=np.int32).reshape(-1, 3),
            "k": ref["k"].astype(np.int32), "code": ref["code"].astype(np.int32), "flags": ref["flags"].astype(np.int32),
            "s": ref["s"], "m": ref["m"]}


def scale_ref(z, beta):
    """``slnlp_scale_logp``'s rows in fp64, rounded once to float32: (beta z - a) - log1p(sum e - 1)."""
    zz = np.asarray(z, dtype=np.float32).astype(np.float64)
    zmax = zz.max(axis=1, keepdims=True)
    at_max = zz == zmax
    e = np.where(at_max, 0.0, np.exp(beta * zz - beta * zmax))
    l = np.log1p(e.sum(axis=1, keepdims=True) + (at_max.sum(axis=1, keepdims=True) - 1.0))
    return ((beta * zz - beta * zmax) - l).astype(np.float32)
