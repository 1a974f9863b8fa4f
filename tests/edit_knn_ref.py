"""numpy / python restatement of csrc/edit_knn.hip (include/slnlp.h states the definitions): unit-cost Levenshtein distances by the
plain two-row dynamic program, the k nearest references by ``np.lexsort((index, distance))`` with exclusion and eligibility, and
the fp64 vote summed in list order.  Nothing here shares code with the library."""
import numpy as np

MAX_LEN = 64
NONE = 255
CODE_QUERY, CODE_EXCLUDE = 1, 2


def levenshtein(a, b):
    """The unit-cost edit distance of two token sequences: the textbook dynamic program, two rows."""
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
        prev = cur
    return prev[len(b)]


def usable(L, width):
    """Which rows take part: a length in 0..min(64, the row's width)"""
    L = np.asarray(L, dtype=np.int64)
    return (L >= 0) & (L <= min(MAX_LEN, int(width)))


def _against_all(q, R, lr):
    """``levenshtein(q, R[j, :lr[j]])`` for every j: the same two rows, each formed for all references at once.  The row's
    left-to-right dependency cur[j] = min(., cur[j - 1] + 1) is min over l <= j of (t[l] + j - l), a running minimum of t - j."""
    nr, S = R.shape
    ar = np.arange(S + 1, dtype=np.int64)
    prev = np.broadcast_to(ar, (nr, S + 1)).copy()
    for i in range(1, len(q) + 1):
        t = np.minimum(prev[:, 1:] + 1, prev[:, :-1] + (R != q[i - 1]))
        cur = np.concatenate([np.full((nr, 1), i, dtype=np.int64), t], axis=1)
        prev = np.minimum.accumulate(cur - ar, axis=1) + ar
    return prev[np.arange(nr), lr]


def distances(Xq, Lq, Xr, Lr):
    """uint8 [nq, nr]: the distance of rows ``Xq[i, :Lq[i]]`` and ``Xr[j, :Lr[j]]``, 255 where either row is not usable"""
    Xq, Xr = np.asarray(Xq, dtype=np.int64), np.asarray(Xr, dtype=np.int64)
    Lq, Lr = np.asarray(Lq, dtype=np.int64), np.asarray(Lr, dtype=np.int64)
    okq, okr = usable(Lq, Xq.shape[1]), usable(Lr, Xr.shape[1])
    out = np.full((len(Lq), len(Lr)), NONE, dtype=np.uint8)
    cols = np.flatnonzero(okr)
    if cols.size:
        R, lr = Xr[cols], Lr[cols]
        for i in np.flatnonzero(okq):
            out[i, cols] = _against_all(Xq[i, :Lq[i]], R, lr)
    return out


def knn_rows(dist, Lq, Lr, q_width, r_width, k, radius=0, exclude=None):
    """The library's three outputs from a distance matrix: {head int64 [8], rows int32 [nq, 4], nbr int32 [nq, k, 2]}"""
    nq, nr = dist.shape
    okq, okr = usable(Lq, q_width), usable(Lr, r_width)
    idx = np.arange(nr)
    head = np.zeros(8, dtype=np.int64)
    head[0], head[1] = (~okq).sum(), (~okr).sum()
    rows = np.zeros((nq, 4), dtype=np.int32)
    nbr = np.full((nq, k, 2), -1, dtype=np.int32)
    for i in range(nq):
        code, ex = 0 if okq[i] else CODE_QUERY, -1
        if exclude is not None:
            e = int(exclude[i])
            if 0 <= e < nr:
                ex = e
            elif e != -1:
                code |= CODE_EXCLUDE
        eligible = okr & (idx != ex) & bool(okq[i])
        d = dist[i].astype(np.int64)
        order = np.lexsort((idx, d))
        order = order[eligible[order]][:k]
        nbr[i, :len(order), 0], nbr[i, :len(order), 1] = d[order], order
        rows[i] = (len(order), (eligible & (d <= radius)).sum(), d[eligible].min() if eligible.any() else -1, code)
    return {"head": head, "rows": rows, "nbr": nbr}


def knn_logp(res, Lq, Lr, yr, prior, weights="distance", tau=1.0, normalize=True, lam=1.0):
    """float32 [nq, V] and the count of neighbours whose label lies outside the V classes: the vote of include/slnlp.h in fp64,
    neighbours in list order"""
    prior = np.asarray(prior, dtype=np.float64)
    V, (nq, k, _) = len(prior), res["nbr"].shape
    out = np.full((nq, V), np.nan, dtype=np.float32)
    bad = 0
    for i in range(nq):
        if res["rows"][i, 3] & CODE_QUERY:
            continue
        s, W = np.zeros(V, dtype=np.float64), np.float64(0.0)
        for j in range(int(res["rows"][i, 0])):
            d, r = int(res["nbr"][i, j, 0]), int(res["nbr"][i, j, 1])
            y = int(yr[r])
            if not 0 <= y < V:
                bad += 1
                continue
            w = np.float64(1.0)
            if weights == "distance":
                n = np.float64(max(int(Lq[i]), int(Lr[r]), 1) if normalize else 1)
                w = np.exp(-np.float64(d) / (np.float64(tau) * n))
            W = W + w
            s[y] = s[y] + w
        lam64 = np.float64(lam)
        out[i] = np.log((s + lam64 * prior) / (W + lam64)).astype(np.float32)
    return out, bad


def prior_of(y, V):
    """EditKNN's prior: (n_c + 1) / (N + V)"""
    y = np.asarray(y, dtype=np.int64)
    return (np.bincount(y, minlength=V).astype(np.float64) + 1.0) / (len(y) + V)


def make_rows(rs, n, S, other_tokens, lengths, token):
    """``n`` rows that lie ``S + 3`` tokens apart: the first L tokens of a row drawn by ``token(size)``, everything behind them --
    the rest of the S columns and the three of padding -- drawn from ``other_tokens`` (tokens of the OTHER side's rows), so that a
    read past L changes a distance"""
    X = rs.choice(np.asarray(other_tokens, dtype=np.int64), size=(n, S + 3))
    L = np.asarray(lengths, dtype=np.int64)
    for i in range(n):
        m = int(min(max(L[i], 0), S))
        X[i, :m] = token(m)
    return X, L
