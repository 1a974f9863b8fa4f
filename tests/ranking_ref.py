"""The numpy restatement of ``slnlp_ranking_rows`` (include/slnlp.h): the counting definition, literally -- every positive of a
class against every row of its column, O(N P) comparisons -- with the rows, the table and the scores formed in fp64.

For class c the rows with y = c are positives (P), every other row with a label in [0, V) a negative (Q); the score of row j for
class c is z[j, c] as given (the float32 log-prob); numpy's comparisons give the conventions: -0.0 == +0.0, -inf an ordinary value.
Per row i with c = y[i], x = z[i, c]:  gt_neg = #{negatives: z > x}, eq_neg = #{negatives: z == x}, ge_pos = #{positives: z >= x}.
AUC_c = sum_i (2 (Q - gt_neg) - eq_neg) / (2 P Q), AP_c = (1 / P) sum_i ge_pos / (ge_pos + gt_neg + eq_neg).  A class with P = 0,
Q = 0 or a NaN in its column (over the rows with a valid label) is undefined."""
import numpy as np

NAMES = ("auc_macro", "auc_weighted", "ap_macro", "ap_weighted")


def rows_ref(z, y):
    """rows int64 [N, 4] = (gt_neg, eq_neg, ge_pos, code): code 0, -1 for a label outside [0, V), -2 for a row whose own class
    holds a NaN (the counts are 0 for both)."""
    z = np.asarray(z)
    y = np.asarray(y).astype(np.int64)
    N, V = z.shape
    valid = (y >= 0) & (y < V)
    rows = np.zeros((N, 4), dtype=np.int64)
    for i in range(N):
        if not valid[i]:
            rows[i, 3] = -1
            continue
        c = y[i]
        col = z[valid, c]
        if np.isnan(col).any():
            rows[i, 3] = -2
            continue
        x = z[i, c]
        pos = y[valid] == c
        rows[i, :3] = (int((col[~pos] > x).sum()), int((col[~pos] == x).sum()), int((col[pos] >= x).sum()))
    return rows


def table_ref(z, y, rows=None):
    """table float64 [V + 1, 4]: row c = (P, NaN entries of column c over the valid rows, sum (2 (Q - gt) - eq), sum ge / (ge + gt +
    eq)), the sums 0 for a class with a NaN; row V = (valid rows, bad labels, 0, 0)."""
    z = np.asarray(z)
    y = np.asarray(y).astype(np.int64)
    N, V = z.shape
    rows = rows_ref(z, y) if rows is None else np.asarray(rows).astype(np.int64)
    valid = (y >= 0) & (y < V)
    nvalid = int(valid.sum())
    table = np.zeros((V + 1, 4))
    table[V, :2] = (nvalid, N - nvalid)
    for c in range(V):
        mine = valid & (y == c)
        P = int(mine.sum())
        table[c, 0] = P
        table[c, 1] = int(np.isnan(z[valid, c]).sum())
        if table[c, 1] > 0 or P == 0:
            continue
        gt, eq, ge = (rows[mine, k].astype(np.float64) for k in range(3))
        table[c, 2] = float(np.sum(2.0 * ((nvalid - P) - gt) - eq))
        table[c, 3] = float(np.sum(ge / (ge + gt + eq)))
    return table


def summary_ref(table):
    """The four scores, ``classes_scored`` and the per-class auc / ap / support from a table."""
    table = np.asarray(table, dtype=np.float64)
    V = table.shape[0] - 1
    auc, ap = np.full(V, np.nan), np.full(V, np.nan)
    support = table[:V, 0].astype(np.int64)
    for c in range(V):
        P, Q = table[c, 0], table[V, 0] - table[c, 0]
        if P > 0 and Q > 0 and table[c, 1] == 0:
            auc[c] = table[c, 2] / (2.0 * P * Q)
            ap[c] = table[c, 3] / P
    d = ~np.isnan(auc)
    out = {k: float("nan") for k in NAMES}
    if d.any():
        w = support[d].astype(np.float64)
        out = {"auc_macro": float(np.mean(auc[d])), "auc_weighted": float(np.sum(auc[d] * w) / np.sum(w)),
               "ap_macro": float(np.mean(ap[d])), "ap_weighted": float(np.sum(ap[d] * w) / np.sum(w))}
    out.update(classes_scored=int(d.sum()), auc=auc, ap=ap, support=support)
    return out


def ranking_ref(z, y):
    """(rows, table, summary) of ``z`` [N, V] and ``y`` [N]."""
    rows = rows_ref(z, y)
    table = table_ref(z, y, rows)
    return rows, table, summary_ref(table)


def make_scores(N, V, seed, quantum=None, absent=()):
    """float32 log-probs [N, V] (log-softmax of random logits that lean towards the label) and labels that never take the classes
    in ``absent``.  ``quantum``: the log-probs are rounded to multiples of it, which forces ties across rows."""
    rs = np.random.RandomState(seed)
    allowed = np.array([c for c in range(V) if c not in set(absent)] or [0])
    y = allowed[rs.randint(0, len(allowed), size=N)].astype(np.int64)
    logits = rs.randn(N, V)
    if V > 1:
        logits[np.arange(N), y] += 1.0
    z = logits - np.log(np.exp(logits).sum(axis=1, keepdims=True))
    if quantum:
        z = np.round(z / quantum) * quantum
    return z.astype(np.float32), y
