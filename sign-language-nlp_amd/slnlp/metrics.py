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

* ``CALIBRATION``: ``neg_ece`` (expected calibration error over 15 equal-width bins of the top-class probability; ``neg_ece<B>``
  for 1 <= B <= 64 bins), ``neg_mce`` (the largest bin's gap, 15 bins) and ``neg_brier`` (the multiclass Brier score
  sum_c (p_c - 1[c = y])^2, mean over the samples) -- from ``slnlp_reliability_rows`` (csrc/reliability.hip), one call per
  distinct bin count and only when such a name is asked for.  The bins are (b / B, (b + 1) / B], closed on the right (Guo et
  al. 2017).  sklearn has no scorer of these names (its ``neg_brier_score`` is binary only).

* ``RANKING``: ``auc_macro`` / ``auc_weighted`` (one-vs-rest ROC AUC per class) and ``ap_macro`` / ``ap_weighted`` (average
  precision per class), averaged over the DEFINED classes -- plainly, or weighted by the class's support -- from
  ``slnlp_ranking_rows`` (csrc/ranking.hip), one call and only when such a name is asked for.  A class is undefined when it has
  no positive or no negative row (a fold of a long-tailed label set lacks classes: sklearn's ``roc_auc_ovr`` is NaN or raises
  there) or when its column holds a NaN; it is left out of both averages, and the score is NaN when no class is defined.
  Per class the numbers are sklearn's binary ``roc_auc_score`` (Mann-Whitney, half credit for ties) and
  ``average_precision_score`` (step-wise; tied positives share a threshold).  They are no means over rows and have no
  bootstrap interval.  ``roc_auc_ovr`` itself stays an sklearn name.

Beside the scorers: ``selective_report`` (the risk-coverage curve, AURC and the level tables from ``slnlp_selective_rows`` /
``_counts``, csrc/selective.hip), ``binomial_upper`` and ``guaranteed_threshold`` (a rejection threshold for a target error rate)
serve ``LogProbJudge.risk_coverage`` / ``fit_rejection``; they are no ``scoring`` names.

Log-probs on the CPU are reduced by a numpy expression instead (``reduce_rows``, ``reliability_numpy``, ``ranking_numpy``); a
scorer name outside the four families goes through sklearn as before.

One documented difference: the rank is taken among the float32 LOG-PROBS.  An sklearn scorer fed ``exp(logp)`` can see
extra ties where two different log-probs round to the same probability, and then orders those classes by index; the
top-k numbers here are sklearn's on the log-probs themselves (which is what the tests compare with).

The ``RANKING`` numbers follow the same convention: the score of a sample for class c is the float32 LOG-PROB z[:, c] as stored,
and ties are ties of those float32 values (-0.0 equals +0.0, -inf is an ordinary value).  A ``ScoringWrapper`` of the same name
ranks ``predict_proba``'s float32 probabilities, where two different log-probs may round to one probability.

Another, of the same kind: the history's ``CALIBRATION`` numbers are taken on the float32 LOG-PROBS, in fp64 (softmax of the row,
maximum subtracted).  A ``ScoringWrapper`` of the same name is fed ``predict_proba``'s float32 PROBABILITIES, which it
renormalises per row in fp64: the two agree to about float32 rounding of a probability (1e-7), not bit for bit, and a
sample whose confidence sits within that distance of a bin edge may change bins.
"""
import math
import re

import numpy as np
import torch

FAST = ("accuracy", "precision_weighted", "recall_weighted", "f1_weighted", "neg_log_loss")
REDUCED = ("precision_macro", "recall_macro", "f1_macro", "balanced_accuracy", "top_k_accuracy")
CALIBRATION = ("neg_ece", "neg_mce", "neg_brier")
RANKING = ("auc_macro", "auc_weighted", "ap_macro", "ap_weighted")
DEFAULT_BINS, MAX_BINS = 15, 64                             # MAX_BINS: SLNLP_REL_MAX_BINS
_TOP_K = re.compile(r"top([1-9][0-9]*)_accuracy\Z")
_ECE_B = re.compile(r"neg_ece([0-9]+)\Z")


def top_k_of(name):
    """k of ``top_k_accuracy`` (2, sklearn's default) / ``top<k>_accuracy``, None for any other name."""
    if name == "top_k_accuracy":
        return 2
    m = _TOP_K.match(name) if isinstance(name, str) else None
    return int(m.group(1)) if m else None


def calibration_metric_of(name):
    """(kind, bins) of a ``CALIBRATION`` name -- ("ece", 15), ("ece", B) for ``neg_ece<B>``, ("mce", 15), ("brier", None) -- and
    None for any other name.  ``neg_ece<B>`` with B outside 1..64 raises ValueError."""
    if name == "neg_ece":
        return "ece", DEFAULT_BINS
    if name == "neg_mce":
        return "mce", DEFAULT_BINS
    if name == "neg_brier":
        return "brier", None
    m = _ECE_B.match(name) if isinstance(name, str) else None
    if not m:
        return None
    bins = int(m.group(1))
    if not 1 <= bins <= MAX_BINS or m.group(1) != str(bins):
        raise ValueError(f"{name}: the number of bins must be an integer in 1..{MAX_BINS}, written without leading zeros")
    return "ece", bins


def is_reduced(name):
    """Whether ``name`` is scored from the device-side reductions: ``FAST``, ``REDUCED``, a ``top<k>_accuracy``, ``CALIBRATION``
    (``neg_ece<B>`` included) or ``RANKING``.  Not a pure predicate: a ``neg_ece<B>`` whose B lies outside 1..64 raises ValueError
    (``calibration_metric_of``), so that a misspelt bin count fails with its own message wherever the name is first looked at."""
    return (name in FAST or name in REDUCED or name in RANKING or top_k_of(name) is not None
            or calibration_metric_of(name) is not None)


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


def class_report(true_sum, pred_sum, tp_sum):
    """The per-class table of an error analysis from the integer class counts ``slnlp_score_rows`` produces (a confusion
    matrix's row sums, column sums and diagonal), in fp64: ``(report, macro)``.  ``report``: {precision, recall, f1 float64 [V],
    support int64 [V] (rows with that label), predicted int64 [V] (rows with that prediction)} -- sklearn's
    ``precision_recall_fscore_support(labels=all V classes, average=None, zero_division=0)``, the keyword the reference's
    ``ScoringWrapper`` passes: a class that is never predicted has precision 0, one that never occurs recall 0.  ``macro``:
    {precision, recall, f1}: the plain means over ALL V classes (``average="macro"`` with the same labels)."""
    ts, ps, tp = (np.asarray(a) for a in (true_sum, pred_sum, tp_sum))
    if not (ts.ndim == 1 and ts.size >= 1 and ts.shape == ps.shape == tp.shape and all(a.dtype.kind in "iu" for a in (ts, ps, tp))):
        raise ValueError(f"class_report: expected three integer arrays of one length, got shapes {ts.shape}, {ps.shape}, {tp.shape}")
    ts, ps, tp = ts.astype(np.int64), ps.astype(np.int64), tp.astype(np.int64)
    report = {kind: _per_class(kind, tp, ps, ts) for kind in ("precision", "recall", "f1")}
    macro = {kind: float(np.average(v)) for kind, v in report.items()}
    report.update(support=ts, predicted=ps)
    return report, macro


def reliability_from_table(table):
    """The table of ``slnlp_reliability_rows`` (include/slnlp.h), float64 [B + 1, 4] on the host, as a dict.  With M = the sum
    of the counts: ``ece`` = sum_b |sum_correct_b - sum_conf_b| / M, ``mce`` = the largest |accuracy_b - confidence_b| over the
    non-empty bins, ``brier`` / ``nll`` / ``accuracy`` / ``confidence`` = means over the M scored rows; ``rows`` = M;
    ``bins``: {count int64 [B], confidence [B], accuracy [B]} (NaN in an empty bin).  A row that holds a NaN (``nan_rows``) makes
    ece, mce, brier and nll NaN, as it does ``neg_log_loss``; so does M = 0."""
    table = np.asarray(table, dtype=np.float64)
    B = table.shape[0] - 1
    count, sum_conf, sum_correct = table[:B, 0], table[:B, 1], table[:B, 2]
    M, bad, nans = float(count.sum()), int(table[B, 2]), int(table[B, 3])
    filled = count > 0
    safe = np.where(filled, count, 1.0)
    conf_b = np.where(filled, sum_conf / safe, np.nan)
    acc_b = np.where(filled, sum_correct / safe, np.nan)
    nan = float("nan")
    out = {"ece": nan, "mce": nan, "brier": nan, "nll": nan, "accuracy": nan, "confidence": nan, "rows": int(M), "bad_labels": bad,
           "nan_rows": nans, "bins": {"count": count.astype(np.int64), "confidence": conf_b, "accuracy": acc_b}}
    if M > 0:
        out["accuracy"], out["confidence"] = float(sum_correct.sum() / M), float(sum_conf.sum() / M)
    if M > 0 and nans == 0:
        out["ece"] = float(np.abs(sum_correct - sum_conf).sum() / M)
        out["mce"] = float(np.abs(acc_b[filled] - conf_b[filled]).max())
        out["brier"], out["nll"] = float(table[B, 0] / M), float(table[B, 1] / M)
    return out


def reliability_numpy(proba, y, bins=DEFAULT_BINS):
    """(rows float64 [N, 4], table float64 [bins + 1, 4]) as ``slnlp_reliability_rows`` defines them, from PROBABILITIES
    ``proba`` [N, V] on the host: every row is renormalised in fp64 (p = proba_i / sum proba_i), then conf = p at the first
    maximum, brier = sum_c (p_c - 1[c = y])^2, nll = -log p_y, and the same bin rule and row codes."""
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= MAX_BINS:
        raise ValueError(f"reliability: bins={bins!r}, expected an integer in 1..{MAX_BINS}")
    bins = int(bins)
    p = np.asarray(proba).astype(np.float64)
    yy = np.asarray(y).astype(np.int64)
    N, V = p.shape
    idx = np.arange(N)
    rows = np.zeros((N, 4))
    with np.errstate(invalid="ignore", divide="ignore"):
        p = p / p.sum(axis=1, keepdims=True)
        bad = (yy < 0) | (yy >= V)
        broken = ~bad & ~np.isfinite(p).all(axis=1)
        fine = ~bad & ~broken
        pred = p.argmax(axis=1)
        onehot = np.zeros((N, V))
        onehot[idx[fine], yy[fine]] = 1.0
        rows[:, 0] = p[idx, pred]
        rows[:, 1] = ((p - onehot) ** 2).sum(axis=1)
        rows[:, 2] = -np.log(p[idx, np.where(fine, yy, 0)])
        rows[:, 3] = 2.0 * np.clip(np.ceil(rows[:, 0] * bins) - 1.0, 0.0, bins - 1.0) + (pred == yy)
    rows[bad] = (0.0, 0.0, 0.0, -1.0)
    rows[broken] = (np.nan, np.nan, np.nan, -2.0)
    return rows, reliability_table_numpy(rows, bins)


def reliability_table_numpy(rows, bins):
    """The table of ``rows`` [N, 4] (numpy's summation order, not the device's)."""
    code = rows[:, 3].astype(np.int64)
    ok = code >= 0
    b = code[ok] >> 1
    table = np.zeros((bins + 1, 4))
    table[:bins, 0] = np.bincount(b, minlength=bins)
    table[:bins, 1] = np.bincount(b, weights=rows[ok, 0], minlength=bins)
    table[:bins, 2] = np.bincount(b, weights=(code[ok] & 1).astype(np.float64), minlength=bins)
    table[bins] = (rows[ok, 1].sum(), rows[ok, 2].sum(), float((code == -1).sum()), float((code == -2).sum()))
    return table


def reliability_summary(logp, y, bins, out=None):
    """``reliability_from_table`` of one epoch's log-probs at beta = 1: on a GPU one ``ops.reliability_rows`` call (``out``: its
    buffers) and one small download; on the CPU ``reliability_numpy`` of exp(log-prob), taken in fp64."""
    if logp.is_cuda:
        from . import ops
        return ops.reliability_download(ops.reliability_rows(logp if logp.dtype == torch.float32 else logp.float(), y, bins=bins, out=out))
    with np.errstate(over="ignore"):
        proba = np.exp(logp.detach().float().numpy().astype(np.float64))
    return reliability_from_table(reliability_numpy(proba, y.detach().numpy(), bins)[1])


def calibration_score(name, summary):
    """The score ``name`` (a ``CALIBRATION`` name: the NEGATED quantity, greater is better) from ``reliability_from_table``'s dict."""
    return -summary[calibration_metric_of(name)[0]]


def calibration_error(y_true, proba, *, kind, bins=None, labels=None):
    """The POSITIVE quantity behind a ``CALIBRATION`` scorer (``ScoringWrapper`` negates it): ``kind`` "ece" | "mce" | "brier" of
    the probabilities ``proba`` [N, V], whose column c stands for class ``labels[c]`` (None: class c).  With two classes
    sklearn's ``predict_proba`` scorers hand over the second column alone, as a 1-D array: the two columns are rebuilt as
    [1 - p, p], which is what ``log_loss`` does with such input."""
    y_true = np.asarray(y_true)
    proba = np.asarray(proba)
    if proba.ndim == 1:
        proba = np.stack([1.0 - proba.astype(np.float64), proba.astype(np.float64)], axis=1)
    if labels is not None:
        labels = np.asarray(labels)
        if len(labels) != proba.shape[1]:
            raise ValueError(f"neg_{kind}: {len(labels)} labels for {proba.shape[1]} probability columns")
        order = np.argsort(labels, kind="stable")
        pos = np.clip(np.searchsorted(labels[order], y_true), 0, len(labels) - 1)
        y_true = np.where(labels[order][pos] == y_true, order[pos], -1)
    summary = reliability_from_table(reliability_numpy(proba, y_true, bins or DEFAULT_BINS)[1])
    if summary["bad_labels"] > 0:
        raise ValueError(f"neg_{kind}: {summary['bad_labels']} of {len(y_true)} labels lie outside the {proba.shape[1]} classes of the "
                         "probabilities")
    return summary[kind]


def ranking_from_table(table):
    """The table of ``slnlp_ranking_rows`` (include/slnlp.h), float64 [V + 1, 4] on the host, as a dict.  Per class, with P its
    positives and Q = (valid rows) - P its negatives: ``auc`` = table[c, 2] / (2 P Q), ``ap`` = table[c, 3] / P, ``support`` = P;
    a class with P = 0, Q = 0 or a NaN in its column is undefined: NaN in ``auc`` and ``ap``.  ``auc_macro`` / ``ap_macro``: the
    plain means over the defined classes, ``auc_weighted`` / ``ap_weighted``: weighted by P over the defined classes, all NaN
    when ``classes_scored`` (their number) is 0.  ``rows``: the rows with a valid label, ``bad_labels``: the others,
    ``nan_classes``: the classes whose column holds a NaN."""
    table = np.asarray(table, dtype=np.float64)
    if table.ndim != 2 or table.shape[0] < 2 or table.shape[1] != 4:
        raise ValueError(f"ranking_from_table: table has shape {table.shape}, expected [V + 1, 4]")
    V = table.shape[0] - 1
    P, nans = table[:V, 0], table[:V, 1]
    rows, bad = int(table[V, 0]), int(table[V, 1])
    Q = table[V, 0] - P
    defined = (P > 0) & (Q > 0) & (nans == 0)
    auc = np.full(V, np.nan)
    ap = np.full(V, np.nan)
    auc[defined] = table[:V, 2][defined] / (2.0 * P[defined] * Q[defined])
    ap[defined] = table[:V, 3][defined] / P[defined]
    n = int(defined.sum())
    nan = float("nan")
    out = {name: nan for name in RANKING}
    if n:
        w = P[defined]
        out = {"auc_macro": float(auc[defined].sum() / n), "auc_weighted": float((auc[defined] * w).sum() / w.sum()),
               "ap_macro": float(ap[defined].sum() / n), "ap_weighted": float((ap[defined] * w).sum() / w.sum())}
    out.update(classes_scored=n, auc=auc, ap=ap, support=P.astype(np.int64), rows=rows, bad_labels=bad,
               nan_classes=int((nans > 0).sum()))
    return out


def conformal_report(table, state=None, min_support=5):
    """The table of ``slnlp_conformal_summary`` (include/slnlp.h), int64 [V + 1, 4] on the host, as a dict, over the n rows that
    were scored: ``coverage`` (the share whose set holds the label), ``mean_size``, ``median_size`` (the lower median),
    ``empty_rate``, ``singleton_rate``, ``size_hist`` int64 [V + 1]; per class ``support``, ``class_coverage`` and
    ``class_mean_size`` (NaN for a class without rows); ``worst_class_coverage``: the minimum over the classes with at least
    ``min_support`` rows (NaN without one); ``rows`` = n and ``excluded``, the rows left out (a NaN row, a label outside the
    classes).  ``state``: ``slnlp_conformal_quantile``'s four doubles, whose qhat / n / k are passed on as ``qhat``,
    ``calibration_rows`` and ``k``."""
    table = np.asarray(table)
    if table.ndim != 2 or table.shape[0] < 2 or table.shape[1] != 4:
        raise ValueError(f"conformal_report: table has shape {table.shape}, expected [V + 1, 4]")
    if isinstance(min_support, (bool, np.bool_)) or not isinstance(min_support, (int, np.integer)) or min_support < 1:
        raise ValueError(f"conformal_report: min_support={min_support!r}, expected an integer >= 1")
    table = table.astype(np.int64)
    V = table.shape[0] - 1
    support, covered, sizes = table[:V, 0], table[:V, 1], table[:V, 2]
    hist = table[:, 3].copy()
    n = int(support.sum())
    nan = float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        class_cov = np.where(support > 0, covered / support, np.nan)
        class_size = np.where(support > 0, sizes / support, np.nan)
    enough = support >= min_support
    out = {"coverage": float(covered.sum() / n) if n else nan, "mean_size": float(sizes.sum() / n) if n else nan,
           "median_size": int(np.searchsorted(np.cumsum(hist), (n + 1) // 2)) if n else nan,
           "empty_rate": float(hist[0] / n) if n else nan, "singleton_rate": float(hist[1] / n) if n else nan,
           "size_hist": hist, "support": support.copy(), "class_coverage": class_cov, "class_mean_size": class_size,
           "worst_class_coverage": float(class_cov[enough].min()) if enough.any() else nan, "rows": n, "excluded": int(table[V, 0])}
    if state is not None:
        state = np.asarray(state, dtype=np.float64)
        out.update(qhat=float(state[0]), calibration_rows=int(state[1]), k=int(state[2]))
    return out


SEL_TABLE_HEAD, SEL_MAX_LEVELS = 40, 8                        # SLNLP_SEL_TABLE_HEAD, SLNLP_SEL_MAX_LEVELS


def aurc_oracle(n, errors):
    """AURC of the best possible confidence for ``errors`` wrong rows among ``n``: every wrong row behind every right one, no two
    rows tied -- (1 / n) sum_{k = n - E + 1 .. n} (k - n + E) / k; NaN for n = 0."""
    n, E = int(n), int(errors)
    return math.fsum((k - n + E) / k for k in range(n - E + 1, n + 1)) / n if n else float("nan")


def selective_report(kappa, rows, counts, table, risks=(), coverages=(), curve=True):
    """``ops.selective_download``'s pieces (``slnlp_selective_rows`` / ``_counts``, include/slnlp.h) as a dict, over the n included
    rows: ``rows`` = n, ``errors`` = E, ``accuracy``, ``excluded_labels`` / ``excluded_nan`` (rows left out for a label outside the
    classes / for a NaN), ``risk_sum``, ``aurc`` (the mean over the rows of the selective risk at the row's own threshold),
    ``aurc_oracle`` (``aurc_oracle(n, E)``) and ``e_aurc``, their difference; ``coverage_at_risk``: per level of ``risks`` {risk,
    accepted, wrong, coverage, selective_risk, threshold} -- the largest acceptance whose empirical risk is at most the level,
    accepted 0 and a NaN threshold when there is none -- and ``risk_at_coverage``: per level of ``coverages`` {coverage, accepted,
    wrong, achieved_coverage, risk, threshold} -- the smallest acceptance that reaches the level; ``curve`` (None with
    ``curve=False``): the distinct thresholds in descending order as arrays ``threshold``, ``accepted``, ``wrong``, ``coverage``,
    ``risk``.  Every threshold is one of ``kappa``'s values bit for bit.  The empirical levels carry no guarantee
    (``guaranteed_threshold`` gives one)."""
    kappa, rows, counts = np.asarray(kappa, dtype=np.float64), np.asarray(rows), np.asarray(counts)
    table = np.asarray(table, dtype=np.float64)
    if len(risks) > SEL_MAX_LEVELS or len(coverages) > SEL_MAX_LEVELS or table.ndim != 1 or table.size < SEL_TABLE_HEAD:
        raise ValueError(f"selective_report: at most {SEL_MAX_LEVELS} levels each and a table of at least {SEL_TABLE_HEAD} doubles")
    n, E = int(table[0]), int(table[1])
    nan = float("nan")
    inc = np.flatnonzero(counts[:, 0] > 0)                   # the included rows: a row counts itself
    ge, first = np.unique(counts[inc, 0], return_index=True)  # ascending acceptance: descending thresholds
    thr, gw = kappa[inc[first]], counts[inc[first], 1]
    where = {int(g): i for i, g in enumerate(ge)}

    def level(at):
        g, w = int(table[at]), int(table[at + 1])
        return g, w, (float(thr[where[g]]) if g else nan)
    at_risk, at_cov = [], []
    for l, r in enumerate(risks):
        g, w, t = level(8 + 2 * l)
        at_risk.append({"risk": float(r), "accepted": g, "wrong": w, "coverage": g / n if n else nan, "selective_risk": w / g if g else nan,
                        "threshold": t})
    for l, c in enumerate(coverages):
        g, w, t = level(8 + 2 * SEL_MAX_LEVELS + 2 * l)
        at_cov.append({"coverage": float(c), "accepted": g, "wrong": w, "achieved_coverage": g / n if n else nan,
                       "risk": w / g if g else nan, "threshold": t})
    out = {"rows": n, "errors": E, "accuracy": 1.0 - E / n if n else nan, "excluded_labels": int(table[2]), "excluded_nan": int(table[3]),
           "risk_sum": float(table[4]), "aurc": float(table[5]), "aurc_oracle": aurc_oracle(n, E), "coverage_at_risk": at_risk,
           "risk_at_coverage": at_cov, "curve": None}
    out["e_aurc"] = out["aurc"] - out["aurc_oracle"]
    if curve:
        out["curve"] = {"threshold": thr, "accepted": ge.astype(np.int64), "wrong": gw.astype(np.int64),
                        "coverage": ge / n if n else ge.astype(np.float64), "risk": gw / ge}
    return out


LABEL_RANKINGS = ("normalized_margin", "self_confidence")


def label_audit_report(rec, y, rank_by="normalized_margin"):
    """``ops.label_audit_download``'s dict (``slnlp_label_audit``, include/slnlp.h) and the given labels ``y`` int [N] as the
    confident-learning report (Northcutt, Jiang and Chuang 2021), everything from the exact integer joint and the per-row record in
    fp64: ``issues``: the rows with a label issue -- confidently another class than the given one -- most suspicious first, as
    arrays ``row``, ``given``, ``suggested``, ``self_confidence``, ``margin``; ``rank_by`` "normalized_margin" orders them by (m
    ascending, row ascending), "self_confidence" by (s ascending, row ascending).  ``joint`` int64 [V, V], rows the given and
    columns the confident class; ``calibrated_joint`` float64 [V, V]: with r_c the joint's row sums, row c scaled to the class's
    support, joint[c][j] n_c / r_c, or n_c on the diagonal for a class with no confident row (no evidence of noise), all divided by
    the usable rows, so it sums to 1 and its rows to n_c / n; ``noise_rate`` = 1 - its trace.  ``per_class``: arrays ``support``
    (n_c), ``threshold`` (t_c, NaN without rows), ``issues`` (issues given c), ``confident_other`` (rows confidently c but
    labelled otherwise) and ``noise`` (1 - the diagonal's share of row c; NaN without rows).  ``pairs``: the likely label swaps
    (given, suggested, count), largest count first.  ``rows`` (the usable ones), ``bad_labels``, ``nan_rows``, ``unconfident`` (usable
    rows without a confident class) and ``argmax_disagrees`` (usable rows whose arg-max is not the given label)."""
    if rank_by not in LABEL_RANKINGS:
        raise ValueError(f"label_audit_report: rank_by={rank_by!r}, expected one of {LABEL_RANKINGS}")
    y = np.asarray(y).astype(np.int64)
    flags, k = np.asarray(rec["flags"]), np.asarray(rec["k"]).astype(np.int64)
    s, m = np.asarray(rec["s"], dtype=np.float64), np.asarray(rec["m"], dtype=np.float64)
    if y.shape != flags.shape:
        raise ValueError(f"label_audit_report: y has shape {tuple(y.shape)}, the record {tuple(flags.shape)} rows")
    head = [int(v) for v in rec["head"]]
    joint = np.asarray(rec["joint"]).astype(np.int64)
    n = np.asarray(rec["n"]).astype(np.int64)
    V = n.size
    rows = np.flatnonzero(flags & 1)
    rows = rows[np.lexsort((rows, (m if rank_by == "normalized_margin" else s)[rows]))]
    r = joint.sum(axis=1)
    total = int(n.sum())
    scaled = np.zeros((V, V), dtype=np.float64)
    seen = r > 0
    scaled[seen] = joint[seen] * (n[seen] / r[seen])[:, None]
    scaled[~seen, ~seen] = n[~seen]                          # no confident row: the support stays on the diagonal
    with np.errstate(invalid="ignore", divide="ignore"):
        q = scaled / float(total) if total else np.full((V, V), np.nan)
        noise = 1.0 - np.diagonal(q) / q.sum(axis=1)
    off = joint - np.diag(np.diagonal(joint))
    return {"issues": {"row": rows, "given": y[rows], "suggested": k[rows], "self_confidence": s[rows], "margin": m[rows]},
            "rank_by": rank_by, "joint": joint, "calibrated_joint": q, "noise_rate": float(1.0 - np.trace(q)) if total else float("nan"),
            "per_class": {"support": n, "threshold": np.asarray(rec["t"], dtype=np.float64), "issues": off.sum(axis=1),
                          "confident_other": off.sum(axis=0), "noise": noise},
            "pairs": [(int(g), int(c), int(cnt)) for g, c, cnt in np.asarray(rec["pairs"]) if cnt > 0],
            "rows": head[0], "bad_labels": head[1], "nan_rows": head[2], "unconfident": head[3], "argmax_disagrees": head[5]}


DYN_FRAC_BITS = 20                                         # SLNLP_DYN_FRAC_BITS: q and mq are fixed point with 20 fraction bits
TRAIN_DYNAMICS_FIELDS = ("confidence", "variability", "correctness", "aum", "forgetting", "first_learned", "epochs_seen")


def train_dynamics_report(got, labels, rows=None, top=50):
    """``ops.train_dynamics_download``'s dict (``slnlp_train_dynamics_epoch``, include/slnlp.h) as the report of a fit's training
    dynamics, on the host from the exact integers, in fp64.  ``labels`` [N]: the label of every train row (any dtype); ``rows`` int
    [N]: the dataset index of every train row (None: 0 .. N - 1); ``top``: the length of the ranked lists.  Per row, over its
    ``visits`` usable visits, with F = 2^20 (``DYN_FRAC_BITS``):

        confidence = sum_q / (visits F)          the mean probability of the gold class (Swayamdipta et al. 2020)
        variability = sqrt(max(0, sum_q2 / (visits F^2) - confidence^2))           its standard deviation
        correctness = correct_visits / visits    aum = sum_mq / (visits F), the area under the margin (Pleiss et al. 2020)
        forgetting: the epochs the row was right at every visit of the epoch before and not in this one (Toneva et al. 2019)
        first_learned: the first epoch it was right at every visit (-1: never); epochs_seen: the epochs that visited it

    Returned: ``hard`` (lowest confidence first), ``ambiguous`` (highest variability first), ``forgotten`` (most forgetting events
    first, only rows with at least one) and ``low_aum`` (lowest AUM first), each cut at ``top``, ties by row index; ``never_learned``:
    ALL seen rows with first_learned == -1, by row index.  Each is a dict of arrays ``row`` (the dataset index), ``label`` and the
    seven statistics above.  A row no usable visit has reached is in none of them.  Totals: ``rows``, ``rows_seen``,
    ``unforgettable`` (learned, no forgetting event), ``never_learned_rows``, ``forgetting_events``, ``epochs``, ``visits``,
    ``bad_labels``, ``nan_rows``, ``bad_rows`` (the head's skipped visits) and ``overflow`` (a row reached the visit limit: its sums
    may have wrapped).  ``per_class``: arrays over the sorted distinct labels -- ``label``, ``support`` (all its train rows), the
    means of confidence, variability, correctness and aum over its SEEN rows (NaN without one), ``never_learned``,
    ``forgetting``.  ``per_row``: the statistics of every train row as arrays [N] (NaN for an unseen row's four means), with
    ``row``, ``label`` and ``visits``."""
    what = "train_dynamics_report"
    if isinstance(top, (bool, np.bool_)) or not isinstance(top, (int, np.integer)) or top < 0:
        raise ValueError(f"{what}: top={top!r}, expected an integer >= 0")
    visits = np.asarray(got["visits"]).astype(np.int64)
    N = visits.size
    labels = np.asarray(labels)
    rows = np.arange(N, dtype=np.int64) if rows is None else np.asarray(rows).astype(np.int64)
    if labels.shape != (N,) or rows.shape != (N,):
        raise ValueError(f"{what}: labels has shape {tuple(labels.shape)} and rows {tuple(rows.shape)}, the state {N} rows")
    F = float(1 << DYN_FRAC_BITS)
    seen = visits > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(seen, visits, 0).astype(np.float64)
        conf = np.asarray(got["sum_q"]).astype(np.float64) / (v * F)
        var = np.asarray(got["sum_q2"]).astype(np.float64) / (v * (F * F)) - conf * conf
        stats = {"confidence": conf, "variability": np.sqrt(np.maximum(0.0, var)),
                 "correctness": np.asarray(got["correct_visits"]).astype(np.float64) / v,
                 "aum": np.asarray(got["sum_mq"]).astype(np.float64) / (v * F)}
    for name in ("confidence", "variability", "correctness", "aum"):
        stats[name] = np.where(seen, stats[name], np.nan)
    for name in ("forgetting", "first_learned", "epochs_seen"):
        stats[name] = np.asarray(got[name]).astype(np.int64)
    at = np.flatnonzero(seen)

    def entries(which):
        return {"row": rows[which], "label": labels[which], **{name: stats[name][which] for name in TRAIN_DYNAMICS_FIELDS}}

    def ranked(key, among=at):
        return entries(among[np.lexsort((rows[among], key[among]))][:int(top)])
    never = at[stats["first_learned"][at] == -1]
    never = never[np.argsort(rows[never], kind="stable")]
    classes, cls = np.unique(labels, return_inverse=True)
    C = classes.size
    n_seen = np.bincount(cls[at], minlength=C).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        means = {name: np.bincount(cls[at], weights=stats[name][at], minlength=C) / n_seen
                 for name in ("confidence", "variability", "correctness", "aum")}
    head = [int(x) for x in got["head"]]
    return {"hard": ranked(stats["confidence"]), "ambiguous": ranked(-stats["variability"]),
            "forgotten": ranked(-stats["forgetting"], at[stats["forgetting"][at] > 0]), "low_aum": ranked(stats["aum"]),
            "never_learned": entries(never),
            "rows": N, "rows_seen": int(at.size), "never_learned_rows": int(never.size),
            "unforgettable": int(np.count_nonzero((stats["first_learned"][at] != -1) & (stats["forgetting"][at] == 0))),
            "forgetting_events": int(stats["forgetting"][at].sum()), "epochs": head[0], "visits": head[1], "bad_labels": head[2],
            "nan_rows": head[3], "bad_rows": head[4], "overflow": bool(head[6]),
            "per_class": {"label": classes, "support": np.bincount(cls, minlength=C), **means,
                          "never_learned": np.bincount(cls[never], minlength=C),
                          "forgetting": np.bincount(cls[at], weights=stats["forgetting"][at], minlength=C).astype(np.int64)},
            "per_row": {"row": rows, "label": labels, "visits": visits, **stats}}


EDIT_BINS = 65                                             # the distances 0 .. SLNLP_EDIT_MAX_LEN
EDIT_MAX_DISTANCE = 64 * 16                                # SLNLP_EDIT_MAX_LEN * SLNLP_FIELD_MAX_FIELDS: the field metric's bound at F = 16


def _max_distance(what, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= EDIT_MAX_DISTANCE:
        raise ValueError(f"{what}: max_distance={v!r}, expected an integer in 1..{EDIT_MAX_DISTANCE}")
    return int(v) + 1


def _edit_tables(what, rows, nbr, y_query, y_ref):
    rows, nbr = np.asarray(rows), np.asarray(nbr)
    if rows.ndim != 2 or rows.shape[1] != 4 or nbr.ndim != 3 or nbr.shape[0] != rows.shape[0] or nbr.shape[1] < 1 or nbr.shape[2] != 2:
        raise ValueError(f"{what}: rows int32 [nq, 4] and nbr int32 [nq, k >= 1, 2] expected (ops.edit_knn_download), got {rows.shape} and {nbr.shape}")
    y_query, y_ref = np.asarray(y_query), np.asarray(y_ref)
    if y_query.shape != (rows.shape[0],) or y_ref.ndim != 1:
        raise ValueError(f"{what}: y_query has shape {tuple(y_query.shape)} and y_ref {tuple(y_ref.shape)}, the tables hold {rows.shape[0]} queries")
    listed = (nbr[:, :, 1] >= 0) & (nbr[:, :, 1] < y_ref.size) & (np.arange(nbr.shape[1])[None, :] < rows[:, :1])
    return rows.astype(np.int64), nbr.astype(np.int64), y_query, y_ref, listed


def _nearest_hist(nearest, bins=EDIT_BINS):
    hist = np.zeros(bins + 1, dtype=np.int64)
    hist[:bins] = np.bincount(nearest[(nearest >= 0) & (nearest < bins)], minlength=bins)
    hist[bins] = np.count_nonzero(nearest < 0)
    return hist


def knn_report(rows, nbr, y_query, y_ref, head=None, max_distance=64):
    """``ops.edit_knn_download``'s tables (``slnlp_edit_knn_rows``, include/slnlp.h) as a summary of a neighbour search, on the host:
    ``rows`` (queries), ``k``, ``flagged_queries`` (a length outside 0..64: no neighbours), ``no_neighbour`` (unflagged, none found),
    ``nearest_hist`` int64 [66] (the nearest distance 0..64, last bin: none), ``mean_nearest``, ``mean_found``, and per rank
    j < k: ``agreement`` (the share of the queries with a j-th neighbour whose label it carries), ``mean_distance`` and ``listed``
    (how many queries have one); ``accuracy_1nn`` = agreement[0] over ALL unflagged queries (a query without a neighbour is wrong).
    ``head``: the download's head, for ``flagged_references`` and ``bad_labels`` (None: not reported).  Labels of any dtype.
    ``max_distance``: the metric's largest distance -- 64, or 64 F for the tables of ``ops.field_knn_rows`` -- ``nearest_hist`` has
    ``max_distance + 2`` bins."""
    bins = _max_distance("knn_report", max_distance)
    rows, nbr, yq, yr, listed = _edit_tables("knn_report", rows, nbr, y_query, y_ref)
    flagged = (rows[:, 3] & 1) != 0
    nearest = np.where(flagged, -1, rows[:, 2])
    same = np.zeros(listed.shape, dtype=bool)
    same[listed] = yr[nbr[:, :, 1][listed]] == np.broadcast_to(yq[:, None], listed.shape)[listed]
    n_listed = listed.sum(axis=0)
    usable = int((~flagged).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        res = {"rows": int(rows.shape[0]), "k": int(nbr.shape[1]), "flagged_queries": int(flagged.sum()),
               "no_neighbour": int(((rows[:, 0] == 0) & ~flagged).sum()), "nearest_hist": _nearest_hist(nearest, bins),
               "mean_nearest": float(nearest[nearest >= 0].mean()) if (nearest >= 0).any() else float("nan"),
               "mean_found": float(rows[~flagged, 0].mean()) if usable else float("nan"),
               "agreement": same.sum(axis=0) / n_listed, "mean_distance": np.where(listed, nbr[:, :, 0], 0).sum(axis=0) / n_listed,
               "listed": n_listed, "accuracy_1nn": float(same[:, 0].sum() / usable) if usable else float("nan")}
    if head is not None:
        res.update(flagged_references=int(head[1]), bad_labels=int(head[2]))
    return res


def split_audit_report(rows, nbr, y_query, y_ref, radius, top, head=None, max_distance=64):
    """Whether held-out rows have twins among the references (``slnlp.split_audit``), from ``ops.edit_knn_download``'s tables of a
    search of the held-out rows (queries) in the train rows (references), on the host.  A query's NEAREST reference is its first
    listed neighbour (smallest distance, then lowest row).  Returned: ``rows``; ``exact_duplicates`` (nearest distance 0) and
    ``near_duplicates`` (<= ``radius``, the exact ones included); ``conflicting``: near duplicates whose nearest reference carries
    ANOTHER label -- irreducible error, or a label problem no model-based audit sees -- and ``conflicting_exact``;
    ``nearest_hist`` int64 [66]: the nearest distances 0..64 and a last bin for "none"; ``per_class``: arrays over the sorted
    distinct query labels -- ``label``, ``support``, ``duplicated``, ``conflicting``; ``pairs``: up to ``top`` tuples (query row,
    reference row, distance, query label, reference label) of the LISTED neighbours within the radius, smallest distance first,
    ties by query then reference row; ``duplicated`` bool [rows]; ``radius``; ``flagged_queries`` (a length outside 0..64: not
    audited) and ``flagged_references`` (``head``: the download's head; None: 0).  Labels of any dtype.  ``max_distance``: the
    metric's largest distance -- 64, or 64 F for the tables of ``ops.field_knn_rows``: ``radius`` lies in 0..max_distance and
    ``nearest_hist`` has ``max_distance + 2`` bins."""
    what = "split_audit_report"
    bins = _max_distance(what, max_distance)
    for name, v, hi in (("radius", radius, bins - 1), ("top", top, 2 ** 31 - 1)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= v <= hi:
            raise ValueError(f"{what}: {name}={v!r}, expected an integer in 0..{hi}")
    rows, nbr, yq, yr, listed = _edit_tables(what, rows, nbr, y_query, y_ref)
    flagged = (rows[:, 3] & 1) != 0
    has = listed[:, 0] & ~flagged
    nearest = np.where(has, nbr[:, 0, 0], -1)
    near = has & (nearest <= radius)
    exact = has & (nearest == 0)
    other = np.zeros(rows.shape[0], dtype=bool)
    other[has] = yr[nbr[has, 0, 1]] != yq[has]
    classes, cls = np.unique(yq, return_inverse=True)
    C = classes.size
    q, j = np.nonzero(listed & ~flagged[:, None] & (nbr[:, :, 0] <= radius))
    d, r = nbr[q, j, 0], nbr[q, j, 1]
    order = np.lexsort((r, q, d))[:int(top)]
    plain = lambda v: v.item() if hasattr(v, "item") else v        # (an object array of names hands out the names themselves)
    pairs = [(int(q[o]), int(r[o]), int(d[o]), plain(yq[q[o]]), plain(yr[r[o]])) for o in order]
    return {"rows": int(rows.shape[0]), "radius": int(radius), "exact_duplicates": int(exact.sum()), "near_duplicates": int(near.sum()),
            "conflicting": int((near & other).sum()), "conflicting_exact": int((exact & other).sum()), "nearest_hist": _nearest_hist(nearest, bins),
            "per_class": {"label": classes, "support": np.bincount(cls, minlength=C), "duplicated": np.bincount(cls[near], minlength=C),
                          "conflicting": np.bincount(cls[near & other], minlength=C)},
            "pairs": pairs, "duplicated": near, "flagged_queries": int(flagged.sum()),
            "flagged_references": int(head[1]) if head is not None else 0}


_LOG_FACTORIAL = [0.0]                                     # ln i!, grown on demand with math.lgamma


def _log_factorials(k):
    while len(_LOG_FACTORIAL) <= k:
        _LOG_FACTORIAL.append(math.lgamma(len(_LOG_FACTORIAL) + 1.0))
    return np.asarray(_LOG_FACTORIAL[:k + 1])


def binomial_upper(e, k, delta):
    """The Clopper-Pearson upper confidence bound of a binomial proportion: the b with P[Bin(k, b) <= e] = delta -- having seen
    ``e`` errors in ``k`` trials, the error rate is above b with probability at most ``delta`` -- by bisection on the CDF, which
    is summed in log space from ``math.lgamma``'s log-factorials.  1.0 for e >= k."""
    if isinstance(e, (bool, np.bool_)) or isinstance(k, (bool, np.bool_)) or not isinstance(e, (int, np.integer)) or \
            not isinstance(k, (int, np.integer)) or k < 1 or e < 0:
        raise ValueError(f"binomial_upper: e={e!r}, k={k!r}, expected integers with k >= 1 and e >= 0")
    if not isinstance(delta, (int, float, np.integer, np.floating)) or isinstance(delta, (bool, np.bool_)) or not 0.0 < float(delta) < 1.0:
        raise ValueError(f"binomial_upper: delta={delta!r}, expected a number in (0, 1)")
    e, k, delta = int(e), int(k), float(delta)
    if e >= k:
        return 1.0
    lf = _log_factorials(k)
    i = np.arange(e + 1, dtype=np.float64)
    coef = lf[k] - lf[:e + 1] - lf[k - e:][::-1]              # ln C(k, i), i = 0 .. e
    log_delta = math.log(delta)

    def log_cdf(b):
        t = coef + i * math.log(b) + (k - i) * math.log1p(-b)
        m = float(t.max())
        return m + math.log(float(np.exp(t - m).sum()))
    lo, hi = 0.0, 1.0                                         # the CDF falls from 1 at b = 0 to 0 at b = 1
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            return hi
        if log_cdf(mid) > log_delta:
            lo = mid
        else:
            hi = mid


def guaranteed_threshold(curve, target_risk, delta=0.05):
    """Pick the rejection threshold of a risk-coverage ``curve`` (``selective_report``'s: distinct thresholds in descending
    order with ``accepted`` and ``wrong``) for a target selective risk.  With ``delta``: the SGR search of Geifman and El-Yaniv
    (2017) -- a binary search over the m distinct thresholds of at most ``steps = max(1, ceil(log2 m))`` probes, each tested with
    ``binomial_upper(wrong, accepted, delta / steps)``; a probe whose bound is at most ``target_risk`` is kept and the search moves
    towards more coverage, another moves it towards less.  On rows drawn like the ones the threshold will be used on, and that the
    fit never saw, the true selective risk at the returned threshold exceeds ``target_risk`` with probability at most ``delta``.
    ``delta=None`` selects the ``empirical`` rule instead: the largest coverage whose empirical risk is at most the target; it
    carries NO guarantee (it overshoots the target about every other time).  Returns {rule, index, threshold, accepted, wrong,
    coverage, risk, bound (None for the empirical rule), steps}, or None when no probe / no threshold qualifies."""
    if not isinstance(target_risk, (int, float, np.integer, np.floating)) or isinstance(target_risk, (bool, np.bool_)) or \
            not 0.0 < float(target_risk) < 1.0:
        raise ValueError(f"guaranteed_threshold: target_risk={target_risk!r}, expected a number in (0, 1)")
    if delta is not None and (not isinstance(delta, (int, float, np.integer, np.floating)) or isinstance(delta, (bool, np.bool_))
                              or not 0.0 < float(delta) < 1.0):
        raise ValueError(f"guaranteed_threshold: delta={delta!r}, expected a number in (0, 1) or None")
    accepted, wrong = np.asarray(curve["accepted"]), np.asarray(curve["wrong"])
    m = int(accepted.size)
    target = float(target_risk)
    pick, bound, steps = None, None, 0
    if delta is None:
        ok = np.flatnonzero(wrong <= target * accepted)
        pick = int(ok[-1]) if ok.size else None              # accepted ascends along the curve
    elif m:
        steps = max(1, int(math.ceil(math.log2(m))))
        lo, hi = 0, m - 1
        for _ in range(steps):
            if lo > hi:
                break
            mid = (lo + hi) // 2
            b = binomial_upper(int(wrong[mid]), int(accepted[mid]), float(delta) / steps)
            if b <= target:
                pick, bound, lo = mid, b, mid + 1
            else:
                hi = mid - 1
    if pick is None:
        return None
    return {"rule": "empirical" if delta is None else "sgr", "index": pick, "threshold": float(curve["threshold"][pick]),
            "accepted": int(accepted[pick]), "wrong": int(wrong[pick]), "coverage": float(curve["coverage"][pick]),
            "risk": float(curve["risk"][pick]), "bound": bound, "steps": steps}


def ranking_numpy(scores, y):
    """(rows int32 [N, 4], table float64 [V + 1, 4]) as ``slnlp_ranking_rows`` defines them, from ``scores`` [N, V] on the host
    (any float dtype: ties are ties of the values as given) and labels ``y`` [N]: per class one sort of the column and two
    ``searchsorted`` per group of rows."""
    z = np.asarray(scores)
    yy = np.asarray(y).astype(np.int64)
    if z.ndim != 2 or yy.shape != (z.shape[0],):
        raise ValueError(f"ranking: scores has shape {z.shape} and y {yy.shape}, expected [N, V] and [N]")
    N, V = z.shape
    ok = (yy >= 0) & (yy < V)
    rows = np.zeros((N, 4), dtype=np.int32)
    rows[~ok, 3] = -1
    table = np.zeros((V + 1, 4))
    nvalid = int(ok.sum())
    table[V, :2] = (nvalid, N - nvalid)
    for c in range(V):
        col = z[ok, c]
        pos = np.flatnonzero(ok & (yy == c))
        P = pos.size
        n_nan = int(np.isnan(col).sum())
        table[c, :2] = (P, n_nan)
        if n_nan:
            rows[pos, 3] = -2
            continue
        if P == 0:
            continue
        x = z[pos, c]
        neg = np.sort(col[yy[ok] != c])
        own = np.sort(x)
        gt = neg.size - np.searchsorted(neg, x, side="right")
        eq = np.searchsorted(neg, x, side="right") - np.searchsorted(neg, x, side="left")
        ge = P - np.searchsorted(own, x, side="left")
        rows[pos, 0], rows[pos, 1], rows[pos, 2] = gt, eq, ge
        Q = nvalid - P
        table[c, 2] = float((2 * (Q - gt.astype(np.int64)) - eq).sum())
        table[c, 3] = float((ge / (ge + gt + eq).astype(np.float64)).sum())
    return rows, table


def ranking_summary(logp, y, out=None):
    """``ranking_from_table`` of one set of log-probs: on a GPU one ``ops.ranking_rows`` call without per-row output (``out``:
    its buffers) and one download of V + 1 rows of four doubles; on the CPU ``ranking_numpy`` of the float32 log-probs."""
    if logp.is_cuda:
        from . import ops
        return ops.ranking_download(ops.ranking_rows(logp if logp.dtype == torch.float32 else logp.float(), y, out=out, per_row=False))
    return ranking_from_table(ranking_numpy(logp.detach().float().numpy(), y.detach().numpy())[1])


def ranking_score(y_true, proba, *, name, labels=None):
    """The ``RANKING`` score ``name`` of the probabilities ``proba`` [N, V], whose column c stands for class ``labels[c]`` (None:
    class c) -- what a ``ScoringWrapper`` of that name calls; a 1-D ``proba`` is the second of two columns, as in
    ``calibration_error``.  Ties are ties of the probabilities as given."""
    y_true = np.asarray(y_true)
    proba = np.asarray(proba)
    if proba.ndim == 1:
        proba = np.stack([1.0 - proba.astype(np.float64), proba.astype(np.float64)], axis=1)
    if labels is not None:
        labels = np.asarray(labels)
        if len(labels) != proba.shape[1]:
            raise ValueError(f"{name}: {len(labels)} labels for {proba.shape[1]} probability columns")
        order = np.argsort(labels, kind="stable")
        pos = np.clip(np.searchsorted(labels[order], y_true), 0, len(labels) - 1)
        y_true = np.where(labels[order][pos] == y_true, order[pos], -1)
    summary = ranking_from_table(ranking_numpy(proba, y_true)[1])
    if summary["bad_labels"] > 0:
        raise ValueError(f"{name}: {summary['bad_labels']} of {len(y_true)} labels lie outside the {proba.shape[1]} classes of the "
                         "probabilities")
    return summary[name]


def epoch_scores(names, logp, y, y_host=None, split=None, out=None, rel_out=None, rank_out=None):
    """{name: score} for the names among ``names`` that ``is_reduced``; ``logp`` / ``y`` are device tensors of one epoch.
    ``split`` names the data in the error a label outside the columns raises; ``out``: ``reduce_rows``' device buffers;
    ``rel_out``: {bins: ``ops.reliability_rows``' device buffers}, one entry per bin count the ``CALIBRATION`` names ask for;
    ``rank_out``: ``ops.ranking_rows``' device buffers (its rows may be None), used when a ``RANKING`` name is asked for."""
    names = [n for n in names if is_reduced(n)]
    if not names:
        return {}
    cal = [n for n in names if calibration_metric_of(n) is not None]
    ranking = [n for n in names if n in RANKING]
    names = [n for n in names if n not in cal and n not in ranking]

    def bad_labels(count):
        return ValueError(f"scoring the {split or 'epoch'} data: {int(count)} of {int(logp.shape[0])} labels lie outside the "
                          f"{int(logp.shape[1])} classes of the log-probs")
    scores = {}
    if names:
        pred, picked, rank, counts = reduce_rows(logp, y, out=out)
        if counts[-1] > 0:
            raise bad_labels(counts[-1])
        y_true = np.asarray(y_host if y_host is not None else y.cpu().numpy()).astype(np.int64)
        scores = scores_from_rows(names, y_true, pred, picked, rank, counts, int(logp.shape[1]))
    summaries = {}
    for name in cal:                                        # history rows are uncalibrated by construction: beta = 1
        bins = calibration_metric_of(name)[1] or DEFAULT_BINS
        if bins not in summaries:
            summaries[bins] = reliability_summary(logp, y, bins, out=(rel_out or {}).get(bins))
            if summaries[bins]["bad_labels"] > 0:
                raise bad_labels(summaries[bins]["bad_labels"])
        scores[name] = calibration_score(name, summaries[bins])
    if ranking:                                             # one call, whatever the number of names; uncalibrated like the rest
        summary = ranking_summary(logp, y, out=rank_out)
        if summary["bad_labels"] > 0:
            raise bad_labels(summary["bad_labels"])
        scores.update({name: summary[name] for name in ranking})
    return scores


# ------------------------------------------------------------------------------------------------------ bootstrap ----
# The fixed columns of ``slnlp_bootstrap_scores``' stats (include/slnlp.h, SLNLP_BOOT_FIXED of them), in order; the value columns
# follow.  ``BOOT_VALUES``: what ``NeuralNetClassifier.score_interval`` forms from ``reliability_rows``' (conf, brier, nll) columns:
# (name, column, sign).
BOOT_COLUMNS = ("accuracy", "precision_macro", "recall_macro", "f1_macro", "precision_weighted", "recall_weighted", "f1_weighted",
                "balanced_accuracy", "top_k_accuracy")
BOOT_VALUES = (("confidence", 0, 1.0), ("neg_brier", 1, -1.0), ("neg_log_loss", 2, -1.0))


def bootstrap_metric_of(name):
    """Where the replicates of the score ``name`` are found in ``slnlp_bootstrap_scores``' stats: ``(column, sign, k)`` -- the
    score is ``sign * stats[:, column]``; ``k`` is the top-k column's k (``top_k_accuracy``: 2, ``top<k>_accuracy``: k), else
    None; the value columns (``BOOT_VALUES``) are counted from ``len(BOOT_COLUMNS)``.  None for a name without an interval
    (ECE and MCE among them: they are no means over rows)."""
    if name in BOOT_COLUMNS[:-1]:
        return BOOT_COLUMNS.index(name), 1.0, None
    k = top_k_of(name)
    if k is not None:
        return len(BOOT_COLUMNS) - 1, 1.0, k
    for value, column, sign in BOOT_VALUES:
        if name == value:
            return len(BOOT_COLUMNS) + column, sign, None
    return None


def _boot_level(what, level):
    if isinstance(level, (bool, np.bool_)) or not isinstance(level, (int, float, np.integer, np.floating)) or not 0.0 < level < 1.0:
        raise ValueError(f"{what}: level={level!r}, expected a number in (0, 1)")
    return float(level)


def _boot_matrix(what, stats, names):
    stats = np.asarray(stats, dtype=np.float64)
    names = list(names)
    if stats.ndim != 2 or stats.shape[0] < 1 or stats.shape[1] != len(names):
        raise ValueError(f"{what}: expected a [replicates, {len(names)}] array for the names {names}, got shape {stats.shape}")
    return stats, names


def _boot_summary(x, level):
    """{mean, std (ddof = 1), lower, upper, n_nan} of the replicates ``x`` that are not NaN (all NaN when there is none)."""
    kept = x[~np.isnan(x)]
    nan = float("nan")
    out = {"mean": nan, "std": nan, "lower": nan, "upper": nan, "n_nan": int(x.size - kept.size)}
    if kept.size:
        alpha = 1.0 - level
        lower, upper = np.quantile(kept, [alpha / 2.0, 1.0 - alpha / 2.0])
        out.update(mean=float(kept.mean()), std=float(kept.std(ddof=1)) if kept.size > 1 else nan, lower=float(lower), upper=float(upper))
    return out


def bootstrap_intervals(stats, names, level=0.95):
    """Percentile bootstrap intervals.  ``stats`` [replicates, len(names)]: one column of replicates per name
    (``ops.bootstrap_scores``' stats, or columns of it).  Per name {mean, std (ddof = 1), lower, upper, n_nan}: ``lower`` and
    ``upper`` are ``np.quantile(x, [alpha / 2, 1 - alpha / 2])``, alpha = 1 - ``level``, over the replicates that are not NaN (a
    replicate without any scored class has no balanced accuracy); ``n_nan`` counts the others.  No replicate left: all four NaN."""
    level = _boot_level("bootstrap_intervals", level)
    stats, names = _boot_matrix("bootstrap_intervals", stats, names)
    return {name: _boot_summary(stats[:, i], level) for i, name in enumerate(names)}


def bootstrap_difference(stats_a, stats_b, names, level=0.95):
    """The paired bootstrap of two fits scored on the SAME resamples (two ``ops.bootstrap_scores`` calls with one seed): per name
    {mean, std, lower, upper, n_nan, p_not_better} of the replicates of ``a - b`` -- ``bootstrap_intervals`` of the difference, plus
    ``p_not_better``: the share of the replicates that are not NaN with ``a - b <= 0`` (all names are scores, greater is better:
    near 0, a beats b by more than resampling noise; 1 for two equal fits).  Raises ValueError when the shapes differ."""
    level = _boot_level("bootstrap_difference", level)
    a, names = _boot_matrix("bootstrap_difference", stats_a, names)
    b, _ = _boot_matrix("bootstrap_difference", stats_b, names)
    if a.shape != b.shape:
        raise ValueError(f"bootstrap_difference: the two sets of replicates differ in shape, {a.shape} and {b.shape}: a paired comparison "
                         "needs the same replicates of the same names")
    out = {}
    for i, name in enumerate(names):
        d = a[:, i] - b[:, i]
        kept = d[~np.isnan(d)]
        out[name] = dict(_boot_summary(d, level), p_not_better=float(np.mean(kept <= 0.0)) if kept.size else float("nan"))
    return out


def uncertainty_summary(rows):
    """An ensemble's per-row uncertainty decomposition -- ``ops.ensemble_rows``' rows float64 [N, 4] = (total entropy, expected
    member entropy, mutual information, disagreeing members), code -2 in the last column for a row that held a NaN -- reduced
    on the host, in fp64, to means over the scored rows: {total_entropy, expected_entropy, mutual_information,
    disagreement_rate (the share of rows on which some member's arg-max is not the ensemble's), mean_disagreement (members per
    row), rows, nan_rows}.  No scored row: the means are NaN."""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != 4:
        raise ValueError(f"uncertainty_summary: rows has shape {rows.shape}, expected [N, 4]")
    ok = rows[:, 3] >= 0
    n = int(ok.sum())
    mean = (lambda v: float(np.sum(v) / n)) if n else (lambda v: float("nan"))
    return {"total_entropy": mean(rows[ok, 0]), "expected_entropy": mean(rows[ok, 1]), "mutual_information": mean(rows[ok, 2]),
            "disagreement_rate": mean(rows[ok, 3] > 0), "mean_disagreement": mean(rows[ok, 3]), "rows": n, "nan_rows": int((~ok).sum())}


def attribution_report(rec, unit_names=None):
    """``ops.attribution_download``'s dict (``slnlp_attribution_summary``, include/slnlp.h) as the report of an occlusion
    attribution, in fp64 from the device's exact counts and fixed-order sums:

    * per row, arrays [N]: ``top_unit`` (the unit whose occlusion lowers the target's log-prob most, -1 for none), ``top_drop``,
      ``min_drop``, ``sum_drop``, ``flips`` (variants whose arg-max is not the base's), ``units`` (usable variants), ``base_pred``,
      ``target`` (-1 for none), ``base_logp`` (the base log-prob of the target);
    * ``per_bin`` over all classes and ``per_class`` per (class, bin), each {mean_drop, mean_kl, flip_rate, count, nonfinite}:
      arrays [n_bins] and [V, n_bins].  ``count`` holds the usable variants whose drop and kl are finite -- the ones in the means --,
      ``nonfinite`` the other usable ones; ``flip_rate`` = flips / (count + nonfinite); a cell with count 0 has NaN means, one
      without a usable variant a NaN flip rate.  The bins' sums over the classes are ``math.fsum``s of the cells;
    * ``ranking``: the bins with a count by mean drop, largest first (ties by ascending bin), as (bin, name, mean_drop);
    * ``unit_names``: the bins' names (``unit_names``, default their numbers as strings), and the head's counts ``variants``,
      ``usable``, ``bad_labels``, ``nonfinite_rows``, ``invalid``, ``flips``."""
    ti, td = np.asarray(rec["table_i"], dtype=np.int64), np.asarray(rec["table_d"], dtype=np.float64)
    ri, rd, head = np.asarray(rec["rows_i"]), np.asarray(rec["rows_d"], dtype=np.float64), np.asarray(rec["head"], dtype=np.int64)
    V, nb = ti.shape[:2]
    names = [str(b) for b in range(nb)] if unit_names is None else [str(u) for u in unit_names]
    if len(names) != nb:
        raise ValueError(f"attribution_report: {len(names)} unit_names for {nb} bins")

    def cells(count, flips, nonfinite, drop, kl):
        count, seen = np.asarray(count, dtype=np.float64), np.asarray(count + nonfinite, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return {"mean_drop": np.where(count > 0, drop / count, np.nan), "mean_kl": np.where(count > 0, kl / count, np.nan),
                    "flip_rate": np.where(seen > 0, flips / seen, np.nan), "count": np.asarray(count, dtype=np.int64),
                    "nonfinite": np.asarray(nonfinite, dtype=np.int64)}
    per_class = cells(ti[:, :, 0], ti[:, :, 1], ti[:, :, 2], td[:, :, 0], td[:, :, 1])
    over = lambda a: np.array([math.fsum(a[:, b]) for b in range(nb)], dtype=np.float64)
    per_bin = cells(ti[:, :, 0].sum(axis=0), ti[:, :, 1].sum(axis=0), ti[:, :, 2].sum(axis=0), over(td[:, :, 0]), over(td[:, :, 1]))
    ranked = sorted((b for b in range(nb) if per_bin["count"][b] > 0), key=lambda b: (-per_bin["mean_drop"][b], b))
    return {"top_unit": ri[:, 5].astype(np.int64), "top_drop": rd[:, 1], "min_drop": rd[:, 2], "sum_drop": rd[:, 3],
            "flips": ri[:, 4].astype(np.int64), "units": ri[:, 3].astype(np.int64), "base_pred": ri[:, 0].astype(np.int64),
            "target": ri[:, 1].astype(np.int64), "base_logp": rd[:, 0], "per_bin": per_bin, "per_class": per_class,
            "ranking": [(b, names[b], float(per_bin["mean_drop"][b])) for b in ranked], "unit_names": names,
            "variants": int(head[:4].sum()), "usable": int(head[0]), "bad_labels": int(head[1]), "nonfinite_rows": int(head[2]),
            "invalid": int(head[3]), "total_flips": int(head[4])}
