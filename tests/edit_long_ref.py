"""numpy / python restatement of csrc/edit_long.hip (include/slnlp.h states the definitions): the search of tests/edit_knn_ref.py
for rows of up to ``max_len`` frames -- unit-cost Levenshtein distances by the plain two-row dynamic program into a uint16 matrix
with 65535 as its "none", usability against min(max_len, the row's width), the selection and the head, and the fp64 vote with the
bound ``max_len``.  ``levenshtein``, ``make_rows``, ``prior_of`` and the vote's arithmetic come from edit_knn_ref (itself not
edited); nothing here shares code with the library."""
import numpy as np

from edit_knn_ref import CODE_EXCLUDE, CODE_QUERY, knn_logp as _vote, levenshtein, make_rows, prior_of  # noqa: F401  (re-exported)

LONG_MAX_LEN = 512
NONE = 65535


def usable(L, width, max_len):
    """Which rows take part: a length in 0..min(max_len, the row's width)"""
    L = np.asarray(L, dtype=np.int64)
    return (L >= 0) & (L <= min(int(max_len), int(width)))


def _against_all(q, R, lr):
    """``levenshtein(q, R[j, :lr[j]])`` for every j: the two rows of the dynamic program, each formed for all references at once.
    The row's left-to-right dependency cur[j] = min(t[j], cur[j - 1] + 1) is min over l <= j of (t[l] + j - l): a running minimum
    of t - j."""
    nr, S = R.shape
    ar = np.arange(S + 1, dtype=np.int64)
    prev = np.broadcast_to(ar, (nr, S + 1)).copy()
    for i in range(1, len(q) + 1):
        t = np.minimum(prev[:, 1:] + 1, prev[:, :-1] + (R != q[i - 1]))
        cur = np.concatenate([np.full((nr, 1), i, dtype=np.int64), t], axis=1)
        prev = np.minimum.accumulate(cur - ar, axis=1) + ar
    return prev[np.arange(nr), lr]


def distances(Xq, Lq, Xr, Lr, max_len):
    """uint16 [nq, nr]: the distance of rows ``Xq[i, :Lq[i]]`` and ``Xr[j, :Lr[j]]``, 65535 where either row is not usable"""
    assert 1 <= max_len <= LONG_MAX_LEN
    Xq, Xr = np.asarray(Xq, dtype=np.int64), np.asarray(Xr, dtype=np.int64)
    Lq, Lr = np.asarray(Lq, dtype=np.int64), np.asarray(Lr, dtype=np.int64)
    okq, okr = usable(Lq, Xq.shape[1], max_len), usable(Lr, Xr.shape[1], max_len)
    out = np.full((len(Lq), len(Lr)), NONE, dtype=np.uint16)
    cols = np.flatnonzero(okr)
    if cols.size:
        R, lr = Xr[cols], Lr[cols]
        for i in np.flatnonzero(okq):
            out[i, cols] = _against_all(Xq[i, :Lq[i]], R, lr)
    return out


def knn_rows(dist, Lq, Lr, q_width, r_width, k, max_len, radius=0, exclude=None):
    """The library's three outputs from a distance matrix: {head int64 [8], rows int32 [nq, 4], nbr int32 [nq, k, 2]}"""
    nq, nr = dist.shape
    okq, okr = usable(Lq, q_width, max_len), usable(Lr, r_width, max_len)
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


def knn_logp(res, Lq, Lr, yr, prior, max_len, weights="distance", tau=1.0, normalize=True, lam=1.0):
    """``edit_knn_ref.knn_logp``'s arithmetic; a neighbour is listed when 0 <= d <= max_len, which every neighbour of ``knn_rows``
    is (asserted: a list with a farther one is not this search's)"""
    found = np.arange(res["nbr"].shape[1])[None, :] < res["rows"][:, :1]
    d = res["nbr"][:, :, 0]
    assert ((d[found] >= 0) & (d[found] <= max_len)).all()
    return _vote(res, Lq, Lr, yr, prior, weights=weights, tau=tau, normalize=normalize, lam=lam)
