"""Numpy restatement of csrc/gloss_structure.hip (include/slnlp.h states the definitions): the structure of the labels of one data
set under an edit distance.  Distances come from ``dup_groups_ref.distances`` (the restatements of the three metrics).

A data set has N rows; label[i] is in 0..C-1, or -1 for a row left out.  d is the N x N matrix, uint8 with the sentinel 255 or
uint16 with 65535.

  n_c              #{j : label[j] = c}
  T[i, c]          for a labelled row i: the sum of d(i, j) over j != i with label[j] = c -- exact integers
  own[i]           T[i, label[i]]
  other_class[i]   among the classes c != label[i] with n_c > 0 the one that minimises T[i, c] / n_c, compared exactly by
                   cross-multiplication in integers, ties to the lower class; -1 if there is none.  other[i] = that class's T, or 0
  class_sum[a, b]  the sum over the rows i of class a of T[i, b]: symmetric; the diagonal counts every within-class pair twice
  medoid[c]        the row of class c with the smallest own[i], ties to the lowest row; -1 for an empty class
  fp64, from those integers (sklearn's ``silhouette_samples``): a = own / (n - 1), b = other / n_other, s = (b - a) / max(a, b);
  s = 0 where the row's class has one member, where there is no other class, or where max(a, b) = 0.  Mean class distance =
  class_sum[a, b] / (n_a n_b), the diagonal class_sum[a, a] / (n_a (n_a - 1)); NaN where the divisor is 0."""
import numpy as np

import dup_groups_ref

HEAD_LABELLED, HEAD_CLASSES, HEAD_LEFT_OUT, HEAD_CODE, HEAD_OWN = 0, 1, 2, 3, 4
TOL = 16 * 2.0 ** -53                                        # a, b and s: a handful of correctly rounded fp64 operations, |s| <= 1

distances = dup_groups_ref.distances


def integers(dist, none, label, C):
    """{own uint32 [N], other uint32 [N], other_class int32 [N], count int32 [C], medoid int32 [C], class_sum int64 [C, C], head
    int64 [8]} of a square distance matrix and labels in -1..C-1.  A sentinel at a pair of two labelled rows is a contract breach:
    AssertionError."""
    dist, label = np.asarray(dist), np.asarray(label, dtype=np.int64)
    N = dist.shape[0]
    assert dist.shape == (N, N) and label.shape == (N,) and label.min() >= -1 and label.max() < C
    lab = label >= 0
    count = np.bincount(label[lab], minlength=C).astype(np.int64)
    d = dist.astype(np.int64)
    assert not (d[np.ix_(lab, lab)] == none)[~np.eye(int(lab.sum()), dtype=bool)].any(), "a sentinel at a labelled pair"
    np.fill_diagonal(d, 0)
    onehot = np.zeros((N, C), dtype=np.int64)
    onehot[np.flatnonzero(lab), label[lab]] = 1
    T = d @ onehot                                           # rows left out are no column of anybody's sum
    T[~lab] = 0
    own, other, other_class = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64), np.full(N, -1, dtype=np.int64)
    for i in np.flatnonzero(lab).tolist():
        own[i] = T[i, label[i]]
        best = -1
        for c in range(C):
            if c == label[i] or count[c] == 0:
                continue
            if best < 0 or int(T[i, c]) * int(count[best]) < int(T[i, best]) * int(count[c]):      # Python integers: exact
                best = c
        if best >= 0:
            other_class[i], other[i] = best, T[i, best]
    class_sum = onehot.T @ T
    medoid = np.full(C, -1, dtype=np.int64)
    for c in range(C):
        rows = np.flatnonzero(label == c)
        if len(rows):
            medoid[c] = rows[np.argmin(own[rows])]           # the first minimum: the lowest row
    assert T.max(initial=0) < 2 ** 32
    head = np.zeros(8, dtype=np.int64)
    head[HEAD_LABELLED], head[HEAD_CLASSES], head[HEAD_LEFT_OUT], head[HEAD_OWN] = lab.sum(), (count > 0).sum(), (~lab).sum(), own.sum()
    return {"own": own.astype(np.uint32), "other": other.astype(np.uint32), "other_class": other_class.astype(np.int32),
            "count": count.astype(np.int32), "medoid": medoid.astype(np.int32), "class_sum": class_sum, "head": head}


def values(label, ints):
    """(a, b, s, class_distance) in fp64 from ``integers``' result; NaN for a row left out"""
    label = np.asarray(label, dtype=np.int64)
    count = ints["count"].astype(np.int64)
    N, C = len(label), len(count)
    a, b, s = np.full(N, np.nan), np.full(N, np.nan), np.full(N, np.nan)
    for i in range(N):
        if label[i] < 0:
            continue
        n, oc = int(count[label[i]]), int(ints["other_class"][i])
        a[i] = float(int(ints["own"][i])) / float(n - 1) if n > 1 else 0.0
        b[i] = float(int(ints["other"][i])) / float(int(count[oc])) if oc >= 0 else 0.0
        top = max(a[i], b[i])
        s[i] = (b[i] - a[i]) / top if n > 1 and oc >= 0 and top > 0 else 0.0
    dist = np.full((C, C), np.nan)
    for x in range(C):
        for y in range(C):
            pairs = int(count[x]) * (int(count[y]) - (x == y))
            if pairs > 0:
                dist[x, y] = float(int(ints["class_sum"][x, y])) / float(pairs)
    return a, b, s, dist


def structure(dist, none, label, C):
    """``integers`` and ``values`` together, with the per-class and the overall mean silhouette"""
    ints = integers(dist, none, label, C)
    a, b, s, cd = values(label, ints)
    label = np.asarray(label, dtype=np.int64)
    lab = label >= 0
    class_s = np.array([s[label == c].mean() if (label == c).any() else np.nan for c in range(C)])
    return dict(ints, a=a, b=b, silhouette=s, class_distance=cd, class_silhouette=class_s,
                mean_silhouette=float(s[lab].mean()) if lab.any() else float("nan"))


def gloss_structure(X, L, y, limit=64, **metric):
    """What ``slnlp.gloss_structure`` computes for the rows (X, L) labelled y: the classes are ``np.unique(y)``, a row whose length
    lies outside 0..min(limit, the row stride) is left out -> (classes, label, ``structure``'s dict)"""
    X, L = np.asarray(X), np.asarray(L)
    classes, label = np.unique(np.asarray(y), return_inverse=True)
    label = np.where((L < 0) | (L > min(limit, X.shape[1])), -1, label.reshape(-1))
    dist, none = distances(X, L, **metric)
    return classes, label, structure(dist, none, label, len(classes))


def clustered_rows(classes, per_class, S, edits, seed):
    """``classes`` glosses of ``per_class`` rows: one random prototype row of S tokens (over 30) per class, every member the
    prototype after at most ``edits`` random substitutions, insertions or deletions -> (X int64 [n, S + edits], L, y), class c's
    rows at c * per_class ..; the labels are c + 2"""
    rs = np.random.RandomState(seed)
    X = np.zeros((classes * per_class, S + edits), dtype=np.int64)
    L = np.zeros(classes * per_class, dtype=np.int64)
    y = np.repeat(np.arange(classes), per_class).astype(np.int64) + 2
    for c in range(classes):
        proto = rs.randint(2, 32, size=S).tolist()
        for m in range(per_class):
            row = list(proto)
            for _ in range(rs.randint(0, edits + 1)):
                kind, at = rs.randint(3), rs.randint(len(row))
                if kind == 0:
                    row[at] = int(rs.randint(2, 32))
                elif kind == 1:
                    row.insert(at, int(rs.randint(2, 32)))
                elif len(row) > 1:
                    del row[at]
            i = c * per_class + m
            X[i, :len(row)], L[i] = row, len(row)
    return X, L, y
