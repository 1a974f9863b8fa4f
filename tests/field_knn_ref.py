"""numpy / python restatement of csrc/field_knn.hip (include/slnlp.h states the definitions): the phonology-weighted edit distance
by the plain two-row dynamic program with ``sub`` and ``gap``, the same program formed for all references at once, the k nearest
references by ``np.lexsort((index, distance))`` with the bound 64 F, and the fp64 vote with the unit F summed in list order.
Nothing here shares code with the library; rows come from ``edit_knn_ref.make_rows``."""
import numpy as np

from edit_knn_ref import CODE_QUERY, CODE_EXCLUDE, MAX_LEN, make_rows, prior_of, usable  # noqa: F401  (re-exported for the tests)

NONE = 65535
MAX_FIELDS = 16


def sub(codes, a, b):
    """The cost of substituting token ``b`` for token ``a``: 0 for the same int64 value, F when either lies outside the table,
    else the number of fields in which their rows of ``codes`` differ (which may be 0)"""
    Vt, F = codes.shape
    a, b = int(a), int(b)
    if a == b:
        return 0
    if not (0 <= a < Vt and 0 <= b < Vt):
        return F
    return int((codes[a] != codes[b]).sum())


def distance(codes, gap, a, b):
    """The weighted edit distance of two token sequences: the textbook dynamic program, two rows."""
    a, b = list(a), list(b)
    prev = [j * gap for j in range(len(b) + 1)]
    for i in range(1, len(a) + 1):
        cur = [i * gap] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + gap, cur[j - 1] + gap, prev[j - 1] + sub(codes, a[i - 1], b[j - 1]))
        prev = cur
    return prev[len(b)]


def _sub_all(codes, a, R):
    """``sub(codes, a, R[j, t])`` for every entry of the int64 matrix ``R``"""
    Vt, F = codes.shape
    inside = (R >= 0) & (R < Vt)
    cost = np.full(R.shape, F, dtype=np.int64)
    if 0 <= int(a) < Vt:
        rows = codes[np.where(inside, R, 0)]                 # [nr, S, F]
        cost = np.where(inside, (rows != codes[int(a)]).sum(axis=2), F)
    return np.where(R == np.int64(a), 0, cost)


def _against_all(codes, gap, q, R, lr):
    """``distance(codes, gap, q, R[j, :lr[j]])`` for every j: the same two rows, each formed for all references at once.  The row's
    left-to-right dependency cur[j] = min(., cur[j - 1] + gap) is a running minimum of cur - j gap."""
    nr, S = R.shape
    ar = np.arange(S + 1, dtype=np.int64) * gap
    prev = np.broadcast_to(ar, (nr, S + 1)).copy()
    for i in range(1, len(q) + 1):
        t = np.minimum(prev[:, 1:] + gap, prev[:, :-1] + _sub_all(codes, q[i - 1], R))
        cur = np.concatenate([np.full((nr, 1), i * gap, dtype=np.int64), t], axis=1)
        prev = np.minimum.accumulate(cur - ar, axis=1) + ar
    return prev[np.arange(nr), lr]


def distances(Xq, Lq, Xr, Lr, codes, gap):
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
            out[i, cols] = _against_all(codes, gap, Xq[i, :Lq[i]], R, lr)
    return out


def knn_rows(dist, Lq, Lr, q_width, r_width, k, F, radius=0, exclude=None):
    """The library's three outputs from a distance matrix: {head int64 [8], rows int32 [nq, 4], nbr int32 [nq, k, 2]}; a distance
    above the bound 64 F is no distance"""
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
        d = dist[i].astype(np.int64)
        eligible = okr & (idx != ex) & bool(okq[i]) & (d <= MAX_LEN * F)
        order = np.lexsort((idx, d))
        order = order[eligible[order]][:k]
        nbr[i, :len(order), 0], nbr[i, :len(order), 1] = d[order], order
        rows[i] = (len(order), (eligible & (d <= radius)).sum(), d[eligible].min() if eligible.any() else -1, code)
    return {"head": head, "rows": rows, "nbr": nbr}


def knn_logp(res, Lq, Lr, yr, prior, F, weights="distance", tau=1.0, normalize=True, lam=1.0):
    """float32 [nq, V] and the count of neighbours whose label lies outside the V classes: the vote of include/slnlp.h in fp64 with
    n = F (normalize ? max(Lq, Lr, 1) : 1), neighbours in list order"""
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
                n = np.float64(F * (max(int(Lq[i]), int(Lr[r]), 1) if normalize else 1))
                w = np.exp(-np.float64(d) / (np.float64(tau) * n))
            W = W + w
            s[y] = s[y] + w
        lam64 = np.float64(lam)
        out[i] = np.log((s + lam64 * prior) / (W + lam64)).astype(np.float32)
    return out, bad
