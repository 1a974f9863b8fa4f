"""numpy restatement of csrc/confusion.hip (``slnlp_topk_rows``, ``slnlp_confusion_matrix``, ``slnlp_confusion_pairs``;
include/slnlp.h states the definitions) and of ``metrics.class_report``.  The top-k order is one ``np.lexsort`` per row, the
probabilities stand on ``calibration_ref._shifted`` like the reliability restatement, the matrix is ``np.add.at`` and the pairs a
stable sort of the off-diagonal cells: what differs from the device is only the order of the sums over the columns and numpy's exp."""
import numpy as np

from calibration_ref import _shifted

TOPK_MAX, CONFUSION_MAX_V, PAIRS_MAX = 64, 4096, 64


def topk_order(row):
    """Every column of one float32 row in the device's total order: a NaN before everything (several by ascending index), then
    larger values first, equal values by ascending index; -inf is an ordinary value."""
    row = np.asarray(row)
    nan = np.isnan(row)
    value = np.where(nan, np.float32(0.0), row)             # (a NaN's own value plays no part: the first key has placed it)
    return np.lexsort((np.arange(len(row)), -value, ~nan))  # the LAST key is the primary one


def topk_ref(logp, k, beta=1.0):
    """(idx int32 [N, k], prob float64 [N, k]) of ``logp`` float32 [N, V] at softmax(beta logp)."""
    logp = np.asarray(logp)
    assert logp.dtype == np.float32 and logp.ndim == 2 and 1 <= k <= min(logp.shape[1], TOPK_MAX)
    idx = np.stack([topk_order(r)[:k] for r in logp]).astype(np.int32)
    z = logp.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        zm = z.max(axis=1)                                  # (a NaN in the row makes it NaN)
        _, e, rest = _shifted(z, beta)                      # e = 1 exactly at the maximum
        prob = np.take_along_axis(e, idx.astype(np.int64), axis=1) / (1.0 + rest)[:, None]
    prob[~np.isfinite(zm)] = np.nan
    return idx, prob


def confusion_ref(pred, y, V):
    """counts int64 [V V + 1]: cell ``y V + pred`` over the rows whose label and prediction lie in [0, V), the rest in the tail."""
    pred, y = np.asarray(pred).astype(np.int64), np.asarray(y).astype(np.int64)
    ok = (y >= 0) & (y < V) & (pred >= 0) & (pred < V)
    counts = np.zeros(V * V + 1, dtype=np.int64)
    np.add.at(counts, y[ok] * V + pred[ok], 1)
    counts[V * V] = int((~ok).sum())
    return counts


def pairs_ref(counts, V, M):
    """pairs int32 [M, 3] = (true, predicted, count): the off-diagonal cells with a count above 0 by count descending, then flat
    index ascending; unused rows (-1, -1, 0)."""
    cells = np.asarray(counts)[:V * V].astype(np.int64)
    flat = np.arange(V * V)
    keep = (cells > 0) & (flat // V != flat % V)
    flat = flat[keep]                                       # ascending
    first = flat[np.argsort(-cells[flat], kind="stable")][:M]
    pairs = np.tile(np.array([-1, -1, 0], dtype=np.int32), (M, 1))
    pairs[:len(first)] = np.stack([first // V, first % V, cells[first]], axis=1)
    return pairs


def class_report_ref(true_sum, pred_sum, tp_sum):
    """({precision, recall, f1, support, predicted}, {precision, recall, f1} macro) with 0 for 0 / 0, the means over all classes."""
    ts, ps, tp = (np.asarray(a).astype(np.float64) for a in (true_sum, pred_sum, tp_sum))
    div = lambda a, b: np.array([x / d if d else 0.0 for x, d in zip(a, b)])
    report = {"precision": div(tp, ps), "recall": div(tp, ts), "f1": div(2.0 * tp, ts + ps)}
    macro = {k: float(np.mean(v)) for k, v in report.items()}
    report.update(support=np.asarray(true_sum).astype(np.int64), predicted=np.asarray(pred_sum).astype(np.int64))
    return report, macro


def handmade_rows():
    """{name: (logp float32 [N, V], y)}: the rows the order rules are checked on -- two NaNs in a row, a -inf column, and 70
    columns that hold only 5 distinct values."""
    from test_calibration_cpu import make_logp
    nan = make_logp(33, 7, 2.0, 0.6, 5)
    nan[0][5, 4] = nan[0][5, 1] = np.nan
    hole = make_logp(33, 7, 2.0, 0.6, 6)
    hole[0][7, (hole[1][7] + 1) % 7] = -np.inf
    five = np.log(np.array([0.05, 0.3, 0.1, 0.35, 0.2], dtype=np.float32))[(np.arange(70) * 3) % 5][None, :]
    five = (five - np.log(np.exp(five.astype(np.float64)).sum())).astype(np.float32)
    return {"two_nans_in_a_row": nan, "one_minus_inf_column": hole, "V70_five_values": (five, np.array([0]))}
