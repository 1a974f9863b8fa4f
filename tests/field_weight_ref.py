"""numpy / python restatement of the per-field weighted edit distance (include/slnlp.h states the definitions) and of the search
that fits the weights: the weighted ``sub``, the plain two-row program, the same program formed for all references at once, the
leave-one-out objective with its fixed summation tree, the cyclic coordinate search with its tie rule, and the synthetic fixture
the search is tried on.  Nothing here shares code with the library.  The selection and the vote are ``field_knn_ref.knn_rows`` /
``knn_logp`` with F := W; rows come from ``edit_knn_ref.make_rows``."""
import math

import numpy as np

from edit_knn_ref import MAX_LEN, make_rows, prior_of, usable  # noqa: F401  (re-exported for the tests)
from field_knn_ref import knn_logp, knn_rows                   # noqa: F401

NONE = 65535
MAX_WEIGHT = 16


def sub(codes, w, a, b):
    """The cost of substituting token ``b`` for token ``a``: 0 for the same int64 value, W = sum(w) when either lies outside the
    table, else the sum of w_f over the fields in which their rows of ``codes`` differ (which may be 0)"""
    Vt, F = codes.shape
    a, b = int(a), int(b)
    if a == b:
        return 0
    if not (0 <= a < Vt and 0 <= b < Vt):
        return int(sum(w))
    return int(sum(int(w[f]) for f in range(F) if codes[a, f] != codes[b, f]))


def distance(codes, w, gap, a, b):
    """The weighted edit distance of two token sequences: the textbook dynamic program, two rows."""
    a, b = list(a), list(b)
    prev = [j * gap for j in range(len(b) + 1)]
    for i in range(1, len(a) + 1):
        cur = [i * gap] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + gap, cur[j - 1] + gap, prev[j - 1] + sub(codes, w, a[i - 1], b[j - 1]))
        prev = cur
    return prev[len(b)]


def _sub_all(codes, w, a, R):
    """``sub(codes, w, a, R[j, t])`` for every entry of the int64 matrix ``R``"""
    Vt, F = codes.shape
    W = int(np.sum(w))
    inside = (R >= 0) & (R < Vt)
    cost = np.full(R.shape, W, dtype=np.int64)
    if 0 <= int(a) < Vt:
        rows = codes[np.where(inside, R, 0)]                 # [nr, S, F]
        cost = np.where(inside, ((rows != codes[int(a)]) * np.asarray(w, dtype=np.int64)).sum(axis=2), W)
    return np.where(R == np.int64(a), 0, cost)


def _against_all(codes, w, gap, q, R, lr):
    """``distance(codes, w, gap, q, R[j, :lr[j]])`` for every j: the two rows formed for all references at once; the row's
    left-to-right dependency cur[j] = min(., cur[j - 1] + gap) is a running minimum of cur - j gap."""
    nr, S = R.shape
    ar = np.arange(S + 1, dtype=np.int64) * gap
    prev = np.broadcast_to(ar, (nr, S + 1)).copy()
    for i in range(1, len(q) + 1):
        t = np.minimum(prev[:, 1:] + gap, prev[:, :-1] + _sub_all(codes, w, q[i - 1], R))
        cur = np.concatenate([np.full((nr, 1), i * gap, dtype=np.int64), t], axis=1)
        prev = np.minimum.accumulate(cur - ar, axis=1) + ar
    return prev[np.arange(nr), lr]


def distances(Xq, Lq, Xr, Lr, codes, w, gap):
    """uint16 [nq, nr]: the distance of rows ``Xq[i, :Lq[i]]`` and ``Xr[j, :Lr[j]]``, 65535 where either row is not usable"""
    Xq, Xr = np.asarray(Xq, dtype=np.int64), np.asarray(Xr, dtype=np.int64)
    Lq, Lr = np.asarray(Lq, dtype=np.int64), np.asarray(Lr, dtype=np.int64)
    codes = np.asarray(codes)
    okq, okr = usable(Lq, Xq.shape[1]), usable(Lr, Xr.shape[1])
    out = np.full((len(Lq), len(Lr)), NONE, dtype=np.uint16)
    cols = np.flatnonzero(okr)
    if cols.size:
        R, lr = Xr[cols], Lr[cols]
        for i in np.flatnonzero(okq):
            out[i, cols] = _against_all(codes, w, gap, Xq[i, :Lq[i]], R, lr)
    return out


# ------------------------------------------------------------------------------------------------------ the objective ----
def tree_sum(values):
    """The fixed tree of ``slnlp_loo_objective``: cell t of 256 adds the values t, t + 256, ... in increasing order, then cells
    t and t + w are added for w = 128, 64, .. 1 -- fp64 throughout, an order that depends on the number of values alone"""
    values = np.asarray(values, dtype=np.float64)
    cell = np.zeros(256, dtype=np.float64)
    for t in range(min(256, len(values))):
        acc = np.float64(0.0)
        for v in values[t::256]:
            acc = acc + v
        cell[t] = acc
    w = 128
    while w >= 1:
        cell[:w] = cell[:w] + cell[w:2 * w]
        w //= 2
    return cell[0]


def loo_objective(logp, y):
    """(rows whose arg-max -- the lowest index on a tie -- is the label, the tree sum of -logp[i, y_i], rows that hold a NaN, rows
    whose label lies outside the classes); a NaN row and a row with such a label are wrong and add nothing"""
    logp, y = np.asarray(logp, dtype=np.float32), np.asarray(y, dtype=np.int64)
    N, V = logp.shape
    nan = np.isnan(logp).any(axis=1)
    bad = ~nan & ((y < 0) | (y >= V))
    ok = ~nan & ~bad
    safe = np.where(ok, y, 0)
    right = ok & (np.argmax(np.where(nan[:, None], 0, logp), axis=1) == safe)
    terms = np.where(ok, -logp[np.arange(N), safe].astype(np.float64), 0.0)
    return int(right.sum()), float(tree_sum(terms)), int(nan.sum()), int(bad.sum())


def loo_logp(X, L, y, V, codes, w, gap, k=5, weights="distance", tau=1.0, normalize=True, lam=1.0):
    """The leave-one-out log-probs of rows judged against themselves: query i skips reference i"""
    W = int(np.sum(w))
    S = X.shape[1]
    dist = distances(X, L, X, L, codes, w, gap)
    res = knn_rows(dist, L, L, S, S, k, W, exclude=np.arange(len(L)))
    return knn_logp(res, L, L, y, prior_of(y, V), W, weights=weights, tau=tau, normalize=normalize, lam=lam)[0]


# ---------------------------------------------------------------------------------------------------------- the search ----
def rank_key(scoring, w, right, total):
    """Smallest first: the lower sum ("neg_log_loss") or the higher count ("accuracy"), then the smaller W, then the
    lexicographically smaller vector"""
    return (total if scoring == "neg_log_loss" else -right, sum(w), tuple(w))


def coordinate_search(F, evaluate, levels=(0, 1, 2, 4), sweeps=2, scoring="neg_log_loss", start=None, reduce=True):
    """Cyclic coordinate search: ``evaluate(w)`` -> (rows right, sum).  Start at all ones (or ``start``); for f = 0..F-1 every
    level for w_f with the others fixed (and the present value where it is no level), candidates with W outside 1..16 skipped,
    the best by ``rank_key`` kept; stop after ``sweeps`` sweeps or one that changed nothing.  Returns {weights (divided by their
    gcd when ``reduce``), unreduced, trace [(field, w, right, sum)], steps, ranked (per step: its candidates as (w, right, sum), best first),
    sweeps_run, converged}"""
    w = tuple(start) if start is not None else (1,) * F
    trace = [(None, w) + tuple(evaluate(w))]
    steps, margins, run, converged = [], [], 0, False
    for _ in range(sweeps):
        changed = False
        for f in range(F):
            values = list(levels) + ([] if w[f] in levels else [w[f]])
            cands = [w[:f] + (v,) + w[f + 1:] for v in values]
            cands = [c for c in cands if 1 <= sum(c) <= MAX_WEIGHT]
            got = [tuple(evaluate(c)) for c in cands]
            trace += [(f, c) + g for c, g in zip(cands, got)]
            order = sorted(range(len(cands)), key=lambda i: rank_key(scoring, cands[i], *got[i]))
            margins.append([(cands[i],) + got[i] for i in order])
            changed |= cands[order[0]] != w
            w = cands[order[0]]
            steps.append(w)
        run += 1
        if not changed:
            converged = True
            break
    g = 0
    for v in w:
        g = math.gcd(g, v)
    return {"weights": tuple(v // g for v in w) if reduce else w, "unreduced": w, "trace": trace, "steps": steps, "ranked": margins,
            "sweeps_run": run, "converged": converged}


# --------------------------------------------------------------------------------------------------------- the fixture ----
def make_fixture(seed, N=60, F=4, values=4, classes=6, frames=8, informative=(0, 2), noise=0.1, drop=0.1, double=0.3):
    """Synthetic rows over F fields of ``values`` values: every class has a prototype of ``frames`` frames; the ``informative``
    fields carry the prototype's value with ``noise`` chance of another one, the other fields are redrawn per row and frame; a
    frame is dropped with chance ``drop`` and one frame is doubled in a ``double`` share of the rows.  Token id = the fields' values as
    digits in base ``values``, so the code table is the digits.  The classes have distinct sizes.  -> (X int64 [N, S], L, y, codes int32 [values ** F, F])"""
    rs = np.random.RandomState(seed)
    Vt = values ** F
    codes = np.stack([(np.arange(Vt) // values ** f) % values for f in range(F)], axis=1).astype(np.int32)
    proto = rs.randint(0, values, size=(classes, frames, F))
    S = frames + 1
    X = np.zeros((N, S), dtype=np.int64)
    L = np.zeros(N, dtype=np.int64)
    # class c gets a share of the rows proportional to c + 5: no two classes share a prior, so two classes with equal votes do not tie
    share = np.arange(classes) + 5.0
    y = np.searchsorted(np.cumsum(share) / share.sum(), (np.arange(N) + 0.5) / N).astype(np.int64)
    rs.shuffle(y)
    for i in range(N):
        row = []
        for t in range(frames):
            if rs.rand() < drop:
                continue
            v = rs.randint(0, values, size=F)
            for f in informative:
                v[f] = proto[y[i], t, f] if rs.rand() >= noise else rs.randint(0, values)
            row.append(int(sum(int(v[f]) * values ** f for f in range(F))))
        if row and rs.rand() < double:
            j = rs.randint(0, len(row))
            row.insert(j, row[j])
        row = row[:S]
        X[i, :len(row)], L[i] = row, len(row)
    return X, L, y, codes
