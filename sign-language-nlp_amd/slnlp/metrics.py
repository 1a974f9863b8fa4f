"""EpochScoring metrics from ONE pass over the epoch's log-probs, which are still on the device.

skorch scores each metric by calling an sklearn scorer on the cached predictions, per metric and per data split:
ten sklearn calls per epoch on an [N, V] probability matrix (neg_log_loss alone binarises the labels into another
[N, V] matrix).  Here the device reduces the epoch to what the metrics are functions of (``slnlp_score_rows``,
csrc/score.hip): per sample the arg-max class, the log-prob of the true class and the rank of the true class among the
row's log-probs (N values each), per class the sums of the confusion matrix's row, column and diagonal.  The scores are
formed on the host with the arithmetic sklearn uses, so the numbers are the ones the sklearn scorers return
(tests/test_pipeline_cpu.py and tests/test_score_cpu.py compare them):

* ``FAST``: the reference's five (config/config-transformer.yaml:9, helper.py:529-554);
* ``REDUCED``: macro precision / recall / F1, balanced accuracy and ``top_k_accuracy`` (k = 2, sklearn's default), plus
  ``top<k>_accuracy`` for any integer 1 <= k < V (``top5_accuracy``).

Log-probs on the CPU are reduced by a numpy expression instead (``reduce_rows``); a scorer name outside the two families
goes through sklearn as before.

One documented difference: the rank is taken among the float32 LOG-PROBS.  An sklearn scorer fed ``exp(logp)`` can see
extra ties where two different log-probs round to the same probability, and then orders those classes by index; the
top-k numbers here are sklearn's on the log-probs themselves (which is what the tests compare with).
"""
import re

import numpy as np
import torch

FAST = ("accuracy", "precision_weighted", "recall_weighted", "f1_weighted", "neg_log_loss")
REDUCED = ("precision_macro", "recall_macro", "f1_macro", "balanced_accuracy", "top_k_accuracy")
_TOP_K = re.compile(r"top([1-9][0-9]*)_accuracy\Z")


def top_k_of(name):
    """k of ``top_k_accuracy`` (2, sklearn's default) / ``top<k>_accuracy``, None for any other name."""
    if name == "top_k_accuracy":
        return 2
    m = _TOP_K.match(name) if isinstance(name, str) else None
    return int(m.group(1)) if m else None


def is_reduced(name):
    """Whether ``name`` is scored from the device-side reduction: ``FAST``, ``REDUCED`` or a ``top<k>_accuracy``."""
    return name in FAST or name in REDUCED or top_k_of(name) is not None


def reduce_epoch(logp, y):
    """Device side: (pred int64 [N], picked float32 [N]) as numpy.  ``logp`` [N, V] log-probs, ``y`` [N] class ids."""
    pred = logp.argmax(1)                                   # first maximum, like numpy
    picked = logp.gather(1, y.view(-1, 1)).view(-1).float()
    return pred.cpu().numpy(), picked.cpu().numpy()


def reduce_rows(logp, y, out=None):
    """(pred int32 [N], picked float32 [N], rank int32 [N], counts int64 [3 V + 1]) as numpy: what ``slnlp_score_rows``
    defines (include/slnlp.h).  ``logp`` on a GPU: one library call and one small download; ``out``: the device buffers
    to reuse (``ops.score_rows``).  ``logp`` on the CPU: the same quantities from numpy."""
    if logp.is_cuda:
        from . import ops
        res = ops.score_rows(logp if logp.dtype == torch.float32 else logp.float(), y, out=out)
        pred, picked, rank, counts = ops.score_download(res)
        return pred, picked, rank, counts.astype(np.int64)
    lp = logp.detach().float().numpy()
    yy = y.detach().numpy().astype(np.int64)
    N, V = lp.shape
    ok = (yy >= 0) & (yy < V)
    ys = np.where(ok, yy, 0)
    picked = lp[np.arange(N), ys].copy()
    picked[~ok] = np.float32(np.nan)
    pred = logp.detach().argmax(1).numpy().astype(np.int32)
    v = picked[:, None]
    with np.errstate(invalid="ignore"):
        rank = (lp > v).sum(1) + ((lp == v) & (np.arange(V)[None, :] > yy[:, None])).sum(1)
    rank = np.where(ok & ~np.isnan(lp).any(1), rank, V).astype(np.int32)
    counts = np.concatenate([np.bincount(yy[ok], minlength=V), np.bincount(pred, minlength=V),
                             np.bincount(yy[ok & (pred == yy)], minlength=V), [int((~ok).sum())]]).astype(np.int64)
    return pred, picked, rank, counts


def _prf(y_true, pred, n_classes):
    true_sum = np.bincount(y_true, minlength=n_classes)
    pred_sum = np.bincount(pred, minlength=n_classes)
    tp_sum = np.bincount(y_true[pred == y_true], minlength=n_classes)
    present = (true_sum + pred_sum) > 0                     # sklearn scores the labels that occur in y_true or y_pred
    return tp_sum[present], pred_sum[present], true_sum[present]


def _prf_counts(counts, n_classes):
    """``_prf`` from the device's class counts."""
    true_sum, pred_sum, tp_sum = (counts[i * n_classes:(i + 1) * n_classes] for i in range(3))
    present = (true_sum + pred_sum) > 0
    return tp_sum[present], pred_sum[present], true_sum[present]


def _divide(num, den):                                      # sklearn _prf_divide with zero_division=0
    den = den.astype(np.float64)
    mask = den == 0.0
    den[mask] = 1.0
    out = num / den
    out[mask] = 0.0
    return out


def _per_class(kind, tp, ps, ts):
    if kind == "precision":
        return _divide(tp, ps)
    if kind == "recall":
        return _divide(tp, ts)
    if kind == "f1":                                        # (1 + b^2) tp / (b^2 true + pred), b = 1
        return _divide(2.0 * tp, 1.0 * ts + ps)
    raise KeyError(kind)


def _scores(names, y_true, pred, picked, n_classes, prf, rank=None):
    """``prf``: () -> (tp_sum, pred_sum, true_sum) over the classes present in ``y_true`` or ``pred``."""
    out = {}
    cache = []
    for name in names:
        k = top_k_of(name)
        if name == "accuracy":                              # accuracy_score: average of (y_true == y_pred)
            out[name] = float(np.average(y_true == pred))
        elif name == "neg_log_loss":
            # log_loss(labels = all classes): probabilities are float32 exp(log-prob), clipped to [eps, 1 - eps] of
            # float32, the log is taken in float64 (xlogy of an int64 indicator and a float32 probability)
            p = np.exp(picked.astype(np.float32))
            eps = np.finfo(np.float32).eps
            p = np.clip(p, eps, 1 - eps)
            out[name] = -float(np.average(-np.log(p.astype(np.float64))))
        elif k is not None:                                 # top_k_accuracy_score: average of the hits
            if rank is None:
                raise KeyError(name)
            if not 1 <= k < n_classes:
                raise ValueError(f"{name}: k={k} must lie in [1, {n_classes}) for {n_classes} classes")
            out[name] = float(np.average(rank < k))
        else:
            if not cache:
                cache.append(prf())
            tp, ps, ts = cache[0]
            if name == "balanced_accuracy":                 # the mean of diag(C) / C.sum(axis=1) over the rows that are not 0 / 0
                seen = ts > 0
                out[name] = float(np.mean(tp[seen] / ts[seen]))
                continue
            kind, _, average = name.partition("_")
            per_class = _per_class(kind, tp, ps, ts)
            if average == "weighted":
                out[name] = float(np.average(per_class, weights=ts)) if ts.sum() > 0 else 0.0
            elif average == "macro":
                out[name] = float(np.average(per_class))
            else:
                raise KeyError(name)
    return out


def scores_from_reduction(names, y_true, pred, picked, n_classes):
    """Host side, from ``reduce_epoch``'s two arrays.  ``names``: ``FAST`` (``REDUCED`` names but the top-k family work too)."""
    return _scores(names, y_true, pred, picked, n_classes, lambda: _prf(y_true, pred, n_classes))


def scores_from_rows(names, y_true, pred, picked, rank, counts, n_classes):
    """Host side, from ``reduce_rows``' four arrays.  ``names``: any for which ``is_reduced`` holds."""
    return _scores(names, y_true, pred, picked, n_classes, lambda: _prf_counts(counts, n_classes), rank=rank)


def epoch_scores(names, logp, y, y_host=None, split=None, out=None):
    """{name: score} for the names among ``names`` that ``is_reduced``; ``logp`` / ``y`` are device tensors of one epoch.
    ``split`` names the data in the error a label outside the columns raises; ``out``: ``reduce_rows``' device buffers."""
    names = [n for n in names if is_reduced(n)]
    if not names:
        return {}
    pred, picked, rank, counts = reduce_rows(logp, y, out=out)
    if counts[-1] > 0:
        raise ValueError(f"scoring the {split or 'epoch'} data: {int(counts[-1])} of {len(pred)} labels lie outside the "
                         f"{int(logp.shape[1])} classes of the log-probs")
    y_true = np.asarray(y_host if y_host is not None else y.cpu().numpy()).astype(np.int64)
    return scores_from_rows(names, y_true, pred, picked, rank, counts, int(logp.shape[1]))
