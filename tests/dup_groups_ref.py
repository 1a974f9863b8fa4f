"""Numpy restatement of csrc/dup_groups.hip (include/slnlp.h states the definitions): the near-duplicate groups of one data set.
Distances come from the restatements of the three metrics -- ``edit_knn_ref.distances``, ``edit_long_ref.distances``,
``field_knn_ref.distances`` (``field_weight_ref.distances`` with per-field weights) -- the components from a plain union-find, and
every row is labelled with the lowest row index of its component."""
import numpy as np

import edit_knn_ref
import edit_long_ref
import field_knn_ref
import field_weight_ref

HEAD_GROUPS, HEAD_PAIRS, HEAD_FLAGGED, HEAD_CODE, HEAD_DEGREES = 0, 1, 2, 3, 4


def distances(X, L, field_codes=None, gap=None, field_weights=None, max_len=None):
    """The N x N matrix of one data set under the metric the arguments name (as ``slnlp.duplicate_groups`` reads them) and its
    sentinel: (uint8, 255) for the unit-cost distance, (uint16, 65535) otherwise"""
    X, L = np.asarray(X, dtype=np.int64), np.asarray(L, dtype=np.int64)
    if field_codes is not None:
        codes = np.asarray(field_codes)
        if field_weights is not None:
            w = np.asarray(field_weights, dtype=np.int64)
            return field_weight_ref.distances(X, L, X, L, codes, w, int(w.sum()) if gap is None else gap), 65535
        return field_knn_ref.distances(X, L, X, L, codes, codes.shape[1] if gap is None else gap), 65535
    if max_len is not None:
        return edit_long_ref.distances(X, L, X, L, max_len), 65535
    return edit_knn_ref.distances(X, L, X, L), 255


def find(parent, x):
    while parent[x] != x:
        x = parent[x]
    return x


def groups(dist, none, radius):
    """{group int32 [N], degree int32 [N], head int64 [8]} of a square distance matrix: an edge joins i != j with dist[i, j] <=
    radius; a row whose own entry is ``none`` is unusable -- a singleton of degree 0, counted in head[2]"""
    dist = np.asarray(dist)
    N = dist.shape[0]
    assert dist.shape == (N, N) and 0 <= radius < none
    parent = list(range(N))
    degree = np.zeros(N, dtype=np.int32)
    flagged = 0
    for i in range(N):
        if dist[i, i] == none:
            flagged += 1
            continue
        for j in np.flatnonzero(dist[i] <= radius).tolist():
            if j == i:
                continue
            degree[i] += 1
            a, b = find(parent, i), find(parent, j)
            if a != b:
                parent[max(a, b)] = min(a, b)                # the root of a tree is its lowest index
    group = np.array([find(parent, i) for i in range(N)], dtype=np.int32)
    head = np.zeros(8, dtype=np.int64)
    head[HEAD_GROUPS] = int((group == np.arange(N)).sum())
    head[HEAD_DEGREES] = int(degree.sum())
    head[HEAD_PAIRS] = head[HEAD_DEGREES] // 2
    head[HEAD_FLAGGED] = flagged
    return {"group": group, "degree": degree, "head": head}


def duplicate_groups(X, L, radius, **metric):
    dist, none = distances(X, L, **metric)
    return groups(dist, none, radius)


def random_rows(n=257, S=12, tokens=4, seed=7):
    """``n`` rows over ``tokens`` tokens, lengths 0..S: short rows over a small alphabet, so that exact and near duplicates abound.
    The columns past a row's length hold tokens too: a read past L changes a distance."""
    rs = np.random.RandomState(seed)
    X = rs.randint(2, 2 + tokens, size=(n, S)).astype(np.int64)
    L = rs.randint(0, S + 1, size=n).astype(np.int64)
    return X, L


def chain_rows(n):
    """Row i: one token repeated i times, so d(i, j) = |i - j|: at radius 1 the deepest trees a hook-to-minimum forest can grow"""
    X = np.full((n, max(n - 1, 1)), 5, dtype=np.int64)
    return X, np.arange(n, dtype=np.int64)


def planted_rows(seed=3, n=300, classes=12, S=10, alter=True):
    """300 rows of 12 glosses whose rows 100..159 are copies of rows 0..59 -- every second copy altered in one token: (X, L, y).
    The originals are random rows over 30 tokens, far apart from each other."""
    rs = np.random.RandomState(seed)
    X = rs.randint(2, 32, size=(n, S)).astype(np.int64)
    L = rs.randint(6, S + 1, size=n).astype(np.int64)
    y = (np.arange(n) % classes).astype(np.int64) + 2
    X[100:160], L[100:160], y[100:160] = X[0:60], L[0:60], y[0:60]
    if alter:
        for i in range(100, 160, 2):
            X[i, 0] = 40 + (i % 3)                           # a token no original holds
    return X, L, y
