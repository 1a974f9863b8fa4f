"""Numpy restatement of ``slnlp_score_rows`` (csrc/score.hip, include/slnlp.h): an epoch's log-probs ``logp`` float32 [N, V]
and labels ``y`` int64 [N] reduced to the five outputs the scoring metrics are functions of.  Written row by row from the
definition, with none of the package's code; the tests hold the kernel and ``slnlp.metrics`` to it with exact equality."""
import numpy as np

QNAN_BITS = 0x7FC00000          # picked[i] of a row whose label is out of range


def score_ref(logp, y):
    """-> (pred int32 [N], picked float32 [N], rank int32 [N], true_sum, pred_sum, tp_sum int32 [V] each, n_bad int)."""
    logp = np.asarray(logp, dtype=np.float32)
    y = np.asarray(y, dtype=np.int64)
    N, V = logp.shape
    pred, picked, rank = np.empty(N, np.int32), np.empty(N, np.float32), np.empty(N, np.int32)
    true_sum, pred_sum, tp_sum = np.zeros(V, np.int32), np.zeros(V, np.int32), np.zeros(V, np.int32)
    n_bad = 0
    for i in range(N):
        row = logp[i]
        nan = np.isnan(row)
        # first maximum; a NaN is larger than everything and the first NaN wins
        p = int(np.flatnonzero(nan)[0]) if nan.any() else int(np.flatnonzero(row == row.max())[0])
        pred[i] = p
        pred_sum[p] += 1
        if not 0 <= y[i] < V:
            picked[i:i + 1].view(np.uint32)[0] = QNAN_BITS
            rank[i] = V
            n_bad += 1
            continue
        c = int(y[i])
        v = row[c]
        picked[i] = v                                       # (a float32 copy: the bits)
        true_sum[c] += 1
        tp_sum[c] += int(p == c)
        if nan.any():
            rank[i] = V
        else:
            rank[i] = int((row > v).sum()) + int((row[c + 1:] == v).sum())
    return pred, picked, rank, true_sum, pred_sum, tp_sum, n_bad


def counts_ref(ref):
    """The kernel's ``counts`` vector [3 V + 1] of ``score_ref``'s result."""
    return np.concatenate([ref[3], ref[4], ref[5], [ref[6]]]).astype(np.int32)


def make_case(N, V, seed=0):
    """Log-probs and labels that exercise every rule, as far as [N, V] has room for them: exact ties at the maximum, ties at the
    true class on both sides of y, a row of all-equal values, -inf entries, a 0.0 / -1e3 row (the log-loss clip case), from 9 rows
    on one NaN row and the labels -1 and V (their rows are the third result), from 12 rows on a NaN at the true class."""
    rs = np.random.RandomState(seed)
    logits = rs.randn(N, V).astype(np.float32) * 2
    logp = (logits - np.log(np.exp(logits.astype(np.float64)).sum(1, keepdims=True))).astype(np.float32)
    logp = np.round(logp * 4) / 4                           # a coarse grid: many natural ties
    y = rs.randint(0, V, size=N).astype(np.int64)
    bad = []
    r = lambda k: k % N                                     # row of rule k: rules share rows when N is small

    if V >= 3:
        i = r(0)                                            # ties at the maximum: the first must win
        logp[i, :] = -3.0
        logp[i, [V // 3, V // 2, V - 1]] = -0.5
        y[i] = V // 2
        i = r(1)                                            # ties at the true class below and above y
        logp[i, :] = np.linspace(-9, -1, V, dtype=np.float32)
        c = V // 2
        y[i] = c
        logp[i, [0, c, V - 1]] = logp[i, c]
    i = r(2)
    logp[i, :] = np.float32(-np.log(V))                     # all equal
    y[i] = min(V - 1, 1)
    i = r(3)
    logp[i, ::2] = -np.inf                                  # -inf entries, the true class among them
    y[i] = 0
    i = r(4)
    logp[i, :] = -1e3                                       # one-hot in probability space
    logp[i, V - 1] = 0.0
    y[i] = 0
    if N >= 6:
        i = r(5)
        logp[i, :] = -np.inf                                # a whole row of -inf: argmax 0
    if N >= 9:
        i = r(6)
        logp[i, V // 2] = np.nan                            # the NaN row, label elsewhere
        logp[i, V - 1] = np.nan
        y[i] = 0
        y[r(7)], y[r(8)] = -1, V
        bad = [r(7), r(8)]
    if N >= 12:
        i = r(9)
        y[i] = 3 % V
        logp[i, y[i]] = np.nan                              # the true class's own log-prob is the NaN
    return logp, y, bad
