"""The numpy fp64 restatement of ``slnlp_conformal_rows`` / ``_quantile`` / ``_summary`` (include/slnlp.h): scores, codes, the
threshold, the sets and the summary table, plus an input maker.  Test infrastructure only.

z float32 log-probs [N, V], beta a number.  p_c = exp(beta z_c - beta zmax) / sum (the columns at the maximum are exp(0) = 1 exactly).
Within a row the classes stand by (value descending, column ascending); rank(c) is 1-based, before(c) the mass in front of c.
LAC: s(c) = 1 - p_c.  APS: s(c) = before(c) + u p_c + lam max(0, rank(c) - k_reg); u = 1, or one draw per row
(``row_u``: word 0 of the Threefry call at counter (row, draw, STAGE, 0) under the key of ``seed``).  Codes: -2 a NaN or a maximum
that is not finite (first), -1 a label outside [0, V), else 0.  k = ceil((n + 1) (1 - alpha)) over the n code-0 rows, qhat the k-th
smallest score, +inf for k > n.  The set: {c : s(c) <= qhat}."""
import math

import numpy as np

from threefry_ref import threefry4x32

ROUNDS = 12                # SLNLP_THREEFRY_ROUNDS
STAGE = 0x636F6E66         # SLNLP_CONFORMAL_STAGE
METHODS = {"lac": 0, "aps": 1}


def row_u(N, seed, draw):
    """float64 [N]: the randomised rows' u, (w + 0.5) 2^-32."""
    seed = int(seed) % (1 << 64)
    idx = np.arange(N, dtype=np.uint32)
    zero = np.zeros_like(idx)
    key = [zero + np.uint32(seed & 0xFFFFFFFF), zero + np.uint32(seed >> 32), zero, zero]
    X = threefry4x32([idx, zero + np.uint32(draw), zero + np.uint32(STAGE), zero], key, ROUNDS)
    return (X[0].astype(np.float64) + 0.5) * 2.0 ** -32


def probs_and_order(z, beta=1.0):
    """(p float64 [N, V], order int64 [N, V]: order[i, m] = the class of rank m + 1, bad bool [N]: rows with code -2)."""
    zz = np.asarray(z, dtype=np.float32).astype(np.float64)
    N, V = zz.shape
    with np.errstate(all="ignore"):
        zmax = zz.max(axis=1)
        bad = ~np.isfinite(zmax) | np.isnan(zz).any(axis=1)
        e = np.exp(beta * zz - (beta * zmax)[:, None])
        p = e / e.sum(axis=1, keepdims=True)
    order = np.lexsort((np.broadcast_to(np.arange(V), (N, V)), -zz), axis=1)     # by -value, then by column
    return p, order, bad


def class_scores(z, beta=1.0, method="aps", lam=0.0, k_reg=0, randomized=False, seed=0, draw=0):
    """(S float64 [N, V]: s(c) of every class, NaN in a row with code -2; rank int64 [N, V]: rank(c); bad bool [N])."""
    p, order, bad = probs_and_order(z, beta)
    N, V = p.shape
    rank = np.empty((N, V), dtype=np.int64)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(1, V + 1), (N, V)), axis=1)
    if METHODS[method] == 0:
        S = 1.0 - p
    else:
        ps = np.take_along_axis(p, order, axis=1)
        before = np.concatenate([np.zeros((N, 1)), np.cumsum(ps, axis=1)[:, :-1]], axis=1)
        u = row_u(N, seed, draw) if randomized else np.ones(N)
        s_sorted = before + u[:, None] * ps + lam * np.maximum(0, np.arange(1, V + 1) - k_reg)[None, :].astype(np.float64)
        S = np.empty((N, V))
        np.put_along_axis(S, order, s_sorted, axis=1)
    S[bad] = np.nan
    return S, rank, bad


def rows_ref(z, y=None, qhat=None, **opts):
    """What ``slnlp_conformal_rows`` writes: {score float64 [N] (None without y), rows int64 [N, 4] = (size, rank(y), covered,
    code), mask bool [N, V] (None without qhat), S, margin: the least |s(c) - qhat| over every class of every row with a set}."""
    S, rank, bad = class_scores(z, **opts)
    N, V = S.shape
    rows = np.zeros((N, 4), dtype=np.int64)
    rows[bad, 3] = -2
    score = None
    ok = np.zeros(N, dtype=bool)
    if y is not None:
        y = np.asarray(y).astype(np.int64)
        inside = (y >= 0) & (y < V)
        rows[~bad & ~inside, 3] = -1
        ok = ~bad & inside
        score = np.full(N, np.nan)
        score[ok] = S[ok, y[ok]]
        rows[ok, 1] = rank[ok, y[ok]]
    mask, margin = None, None
    if qhat is not None:
        with np.errstate(invalid="ignore"):
            mask = S <= qhat                                                     # a NaN row: nothing
        rows[:, 0] = mask.sum(axis=1)
        if y is not None:
            rows[ok, 2] = mask[ok, y[ok]]
        margin = float(np.min(np.abs(S[~bad] - qhat))) if (~bad).any() else float("inf")
    return {"score": score, "rows": rows, "mask": mask, "S": S, "margin": margin}


def pack_sets(mask):
    """bool [N, V] -> uint32 [N, ceil(V / 32)]: bit c & 31 of word c >> 5."""
    N, V = mask.shape
    W = (V + 31) // 32
    padded = np.zeros((N, 32 * W), dtype=np.uint8)
    padded[:, :V] = mask
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").reshape(N, W)


def quantile_ref(score, code, alpha):
    """(qhat, n, k, excluded) over the rows with code 0."""
    code = np.asarray(code)
    s = np.asarray(score, dtype=np.float64)[code == 0]
    n = int(s.size)
    k = math.ceil(float(n + 1) * (1.0 - alpha))
    qhat = float("inf") if k > n else float(np.partition(s, k - 1)[k - 1])
    return qhat, n, k, int(code.size - n)


def summary_ref(rows, y, V):
    """int64 [V + 1, 4]: row c = (rows of class c, covered, sum of sizes) over the code-0 rows; column 3 of row s = the code-0 rows
    with a set of size s; [V, 0] = the other rows."""
    rows = np.asarray(rows).astype(np.int64)
    y = np.asarray(y).astype(np.int64)
    table = np.zeros((V + 1, 4), dtype=np.int64)
    for (size, _, covered, code), c in zip(rows, y):
        if code != 0 or not 0 <= c < V:
            table[V, 0] += 1
            continue
        table[c, 0] += 1
        table[c, 1] += int(covered != 0)
        table[c, 2] += size
        table[size, 3] += 1
    return table


def make_logp(N, V, seed, quantum=None, lean=1.0):
    """float32 log-probs [N, V] (log-softmax of random logits that lean towards the label) and the labels.  ``quantum``: the
    log-probs are rounded to multiples of it, which forces ties inside rows."""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, V, size=N).astype(np.int64)
    logits = rs.randn(N, V)
    if V > 1:
        logits[np.arange(N), y] += lean
    z = logits - np.log(np.exp(logits).sum(axis=1, keepdims=True))
    if quantum:
        z = np.round(z / quantum) * quantum
    return z.astype(np.float32), y


def pick_qhat(S, target, margin=1e-9):
    """A threshold near the ``target`` quantile of the finite entries of ``S`` that no entry comes closer to than ``margin``: the
    midpoint of the widest gap between neighbouring values around the target."""
    v = np.unique(S[np.isfinite(S)])
    if v.size < 2:
        return float(v[0] + 0.25) if v.size else 0.5
    i = int(np.clip(round(target * (v.size - 1)), 0, v.size - 2))
    lo, hi = max(0, i - 8), min(v.size - 1, i + 8)
    gaps = np.diff(v[lo:hi + 1])
    g = int(np.argmax(gaps))
    assert gaps[g] > 2 * margin, "no gap wide enough around the target"
    return float(0.5 * (v[lo + g] + v[lo + g + 1]))
