"""Everything that judges an [N, V] matrix of log-probs, written once: ``LogProbJudge``.

``NeuralNetClassifier`` (one fit), ``VotingEnsemble`` (several, combined on the device), ``PriorShift`` (re-weighted) and
``OutOfFold`` (each row from the fit that did not see it) inherit these methods; a consumer added here exists on all of them.  The mixin is written against one hook and a few attributes of its host class:

* ``self._forward_logp(ds, then)``: the log-probs [len(ds), V] of ``ds`` on the device, handed on the estimator's stream to
  ``then(logp, y_dev)``; returns what ``then`` returns once that stream has drained;
* ``classes_``, ``initialized_``, ``predict_nonlinearity``;
* ``calibration_`` / ``_cal_state`` / ``temperature_``: a fitted temperature and its device state (absent or None: T = 1); ``_cal_bias``:
  the device bias of a ``bias_temperature`` calibration (absent or None: a temperature alone) -- ``_calibrated_logp`` is the one
  place that decides how a consumer gets calibrated log-probs;
* ``conformal_`` / ``_conf_state``: the conformal options and the device threshold, set here by ``_set_conformal``;
* ``rejection_`` / ``_rej_state``: the reject option's threshold and its device state, set here by ``_set_rejection``.

What needs the fit itself and not its log-probs (the valid split, the weights, the checkpoint) stays in slnlp/net.py."""
import math
import warnings

import numpy as np
import torch

from . import metrics, ops
from .data import DeviceRows, TokenDataset


CONFORMAL_DEFAULTS = {"alpha": 0.1, "method": "aps", "randomized": True, "lam": 0.0, "k_reg": 0, "seed": 0}
CONFORMAL_METHODS = tuple(ops._lib.CONFORMAL_METHODS)
SELECTIVE_SCORES = tuple(ops._lib.SEL_SCORES)


def conformal_options(setting):
    """The ``conformal`` setting with its defaults filled in -- {alpha 0.1, method "aps", randomized True, lam 0.0, k_reg 0,
    seed 0} -- or None (off).  ``method``: "lac" (1 - p of the class) or "aps" (the mass in front of the class plus u times its
    own; ``lam`` > 0 with ``k_reg`` adds RAPS' penalty lam max(0, rank - k_reg)).  Anything else raises ValueError here."""
    if setting is None or setting is False:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"conformal={setting!r}: expected a dict with keys among {tuple(CONFORMAL_DEFAULTS)} or None")
    unknown = sorted(set(setting) - set(CONFORMAL_DEFAULTS))
    if unknown:
        raise ValueError(f"conformal: unknown keys {unknown} (known: {tuple(CONFORMAL_DEFAULTS)})")
    o = {**CONFORMAL_DEFAULTS, **setting}
    real = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if not real(o["alpha"]) or not 0.0 < float(o["alpha"]) < 1.0:
        raise ValueError(f"conformal: alpha={o['alpha']!r}, expected a number in (0, 1)")
    if o["method"] not in CONFORMAL_METHODS:
        raise ValueError(f"conformal: method={o['method']!r}, expected one of {CONFORMAL_METHODS}")
    if not isinstance(o["randomized"], (bool, np.bool_)):
        raise ValueError(f"conformal: randomized={o['randomized']!r}, expected True or False")
    if not real(o["lam"]) or not 0.0 <= float(o["lam"]) < float("inf"):
        raise ValueError(f"conformal: lam={o['lam']!r}, expected a finite number >= 0")
    if not whole(o["k_reg"]) or not 0 <= o["k_reg"] < 2 ** 31:
        raise ValueError(f"conformal: k_reg={o['k_reg']!r}, expected an integer >= 0")
    if not whole(o["seed"]) or not 0 <= o["seed"] < 2 ** 64:
        raise ValueError(f"conformal: seed={o['seed']!r}, expected an integer in 0..2^64 - 1")
    return {"alpha": float(o["alpha"]), "method": o["method"], "randomized": bool(o["randomized"]), "lam": float(o["lam"]),
            "k_reg": int(o["k_reg"]), "seed": int(o["seed"])}


def conformal_least_rows(alpha):
    """The least number n of calibration rows with ceil((n + 1)(1 - alpha)) <= n: fewer give an infinite threshold."""
    n = max(1, int(math.ceil((1.0 - alpha) / alpha)) - 2)
    while math.ceil(float(n + 1) * (1.0 - alpha)) > n:
        n += 1
    return n


ATTRIBUTION_DEFAULTS = {"by": "frame", "mode": "mask", "width": 1, "stride": 1, "bins": 8, "target": "label"}
ATTRIBUTION_BY = ("frame", "window", "field")
ATTRIBUTION_MODES = ("mask", "drop")
ATTRIBUTION_TARGETS = tuple(ops._lib.ATTR_TARGETS)


def attribution_options(setting):
    """The ``attribution`` setting with its defaults filled in -- {by "frame", mode "mask", width 1, stride 1, bins 8, target
    "label"} -- or None (off).  ``by``: "frame" (windows of width 1; ``width`` must be 1), "window" or "field" (one unit per
    phonological field; ``mode``, ``width``, ``stride`` and ``bins`` are not used).  Anything else raises ValueError here."""
    if setting is None or setting is False:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"attribution={setting!r}: expected a dict with keys among {tuple(ATTRIBUTION_DEFAULTS)} or None")
    unknown = sorted(set(setting) - set(ATTRIBUTION_DEFAULTS))
    if unknown:
        raise ValueError(f"attribution: unknown keys {unknown} (known: {tuple(ATTRIBUTION_DEFAULTS)})")
    o = {**ATTRIBUTION_DEFAULTS, **setting}
    whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if o["by"] not in ATTRIBUTION_BY:
        raise ValueError(f"attribution: by={o['by']!r}, expected one of {ATTRIBUTION_BY}")
    if o["mode"] not in ATTRIBUTION_MODES:
        raise ValueError(f"attribution: mode={o['mode']!r}, expected one of {ATTRIBUTION_MODES}")
    if o["target"] not in ATTRIBUTION_TARGETS:
        raise ValueError(f"attribution: target={o['target']!r}, expected one of {ATTRIBUTION_TARGETS}")
    for k in ("width", "stride"):
        if not whole(o[k]) or not 1 <= o[k] < 2 ** 31:
            raise ValueError(f"attribution: {k}={o[k]!r}, expected an integer >= 1")
    if not whole(o["bins"]) or not 1 <= o["bins"] <= ops._lib.ATTR_MAX_BINS:
        raise ValueError(f"attribution: bins={o['bins']!r}, expected an integer in 1..{ops._lib.ATTR_MAX_BINS}")
    if o["by"] == "frame" and o["width"] != 1:
        raise ValueError(f"attribution: by='frame' occludes one frame at a time, width={o['width']!r}; use by='window'")
    return {"by": o["by"], "mode": o["mode"], "width": int(o["width"]), "stride": int(o["stride"]), "bins": int(o["bins"]), "target": o["target"]}


CONFORMAL_DRAW_CALIBRATE, CONFORMAL_DRAW_PREDICT = 0, 1    # the u of a row at prediction time is independent of the calibration draws


class LogProbJudge:
    # ---------------------------------------------------------- the preamble
    def _require_initialized(self):
        if not self.initialized_:
            raise RuntimeError("This NeuralNetClassifier instance is not initialized yet.")

    def _uses_temperature(self, calibrated):
        """Whether the probabilities are softmax(z / T) with the fit's temperature: it has one and the caller wants it."""
        return bool(calibrated) and getattr(self, "calibration_", None) is not None

    def _calibrated_logp(self, logp, use):
        """How a consumer gets calibrated log-probs, decided in ONE place: ``(logp, state)`` -- ``state`` is what the consumer passes
        on to its ``ops`` call.  Not ``use``: ``(logp, None)``, T = 1.  A temperature: ``(logp, _cal_state)`` unchanged, the device
        reads beta.  A ``bias_temperature`` calibration: the float32 log-probs become ``(beta z + b) - logsumexp(beta z + b)`` IN
        PLACE (``ops.shift_logp``, on the current stream) and the consumer gets ``state=None``: beta = 1 on what is now calibrated."""
        if not use:
            return logp, None
        bias = getattr(self, "_cal_bias", None)
        if bias is None:
            return logp, self._cal_state
        ops.shift_logp(logp, bias, state=self._cal_state, out=logp)
        return logp, None

    def _calibrated_values(self, logp, use):
        """The calibrated float32 log-probs themselves, in place, for a consumer of the values (``predict_proba``, ``ranking``)."""
        logp, state = self._calibrated_logp(logp, use)
        if state is not None:
            ops.scale_logp(logp, state, out=logp)            # beta z - logsumexp(beta z)
        return logp

    def _report_calibration(self, res, use):
        """``res["calibration"]`` = the method's name, only for a fit whose calibration is more than a temperature."""
        if use and getattr(self, "_cal_bias", None) is not None:
            res["calibration"] = self.calibration_["method"]
        return res

    def _judge(self, ds, then):
        """``_forward_logp`` for the consumers: ``then`` receives float32 log-probs."""
        return self._forward_logp(ds, lambda logp, yd: then(logp if logp.dtype == torch.float32 else logp.float(), yd))

    def _labels(self, what, ds, y, check=False):
        """The labels a consumer judges against -- ``y``, or the dataset's when it is None: ``(host int64 [N], on_device)``;
        ``on_device(logp, y_dev)`` yields them inside ``then`` as a contiguous tensor on the log-probs' device.  ``check``:
        labels outside the classes raise here, before the forward passes; the other consumers read the device's count of them
        afterwards (``_refuse_labels``)."""
        labels = ds.y if y is None else np.ascontiguousarray(np.asarray(y), dtype=np.int64)
        if labels.shape != (len(ds),):
            raise ValueError(f"{what}: y has shape {tuple(labels.shape)}, expected ({len(ds)},)")
        if check:
            self._refuse_labels(what, ((labels < 0) | (labels >= len(self.classes_))).sum(), len(ds), len(self.classes_))
        return labels, lambda logp, yd: (yd if y is None else torch.from_numpy(labels).to(logp.device)).contiguous()

    @staticmethod
    def _refuse_labels(what, bad, n, V):
        if bad > 0:
            raise ValueError(f"{what}: {int(bad)} of {n} labels lie outside the {V} classes of the log-probs")

    @staticmethod
    def _as_dataset(X, y=None):
        if isinstance(X, TokenDataset):
            return X
        if isinstance(X, dict):
            return TokenDataset(X["X"], X["lengths"], X["y"] if y is None else y)
        raise TypeError("X must be a slnlp.data.TokenDataset (ids, lengths and labels travel together: the "
                        "Transformer consumes y as decoder input, transformer.py:65)")

    # --------------------------------------------------------------- predict
    def predict_proba(self, X):
        """softmax of the module output -- the module returns log-probs and skorch's
        ``predict_nonlinearity='auto'`` applies softmax for CrossEntropyLoss."""
        self._require_initialized()

        def scaled(out, yd):
            return self._calibrated_values(out, self._uses_temperature(True))    # softmax(z / T) below: the calibrated log-probs, in place
        out = self._forward_logp(self._as_dataset(X), scaled).cpu()
        # the nonlinearity on the host copy (torch's CPU softmax -- the op the reference's CPU path runs): torch's GPU kernels
        # are built with packed fp32 and must not run beside other fits' kernels (STREAM_MODE above); [N, V] is tiny
        return (torch.softmax(out, dim=-1) if self.predict_nonlinearity == "auto" else out).numpy()

    def predict(self, X):
        """The arg-max of ``predict_proba``.  Under a temperature it is the uncalibrated arg-max; under a ``bias_temperature``
        calibration it is the arg-max of the CALIBRATED probabilities -- consistent with ``predict_proba`` and ``predict_topk`` --
        and can differ from the uncalibrated one: a per-class bias moves it."""
        return self.classes_[self.predict_proba(X).argmax(-1)]

    def reliability(self, X, y=None, bins=15, calibrated=True):
        """Reliability diagnostics of this fit's predictions on ``X`` (``y``: the labels; None: the dataset's), all formed from one
        ``ops.reliability_rows`` call on the device log-probs of ``predict_proba``'s forward passes: ``ops.reliability_download``'s
        dict -- ece, mce (``bins`` equal-width right-closed bins of the top-class probability, 1..64), brier, nll, accuracy,
        confidence, rows, bad_labels, nan_rows, bins {count, confidence, accuracy} -- plus ``temperature``: the T the
        probabilities were taken at, softmax(z / T) -- ``temperature_`` for a calibrated fit unless ``calibrated=False``, else 1.0
        (the device then reads no state)."""
        self._require_initialized()
        bins = ops._int_in("reliability", "bins", bins, 1, metrics.MAX_BINS)
        ds = self._as_dataset(X)
        use = self._uses_temperature(calibrated)
        _, on_device = self._labels("reliability", ds, y)

        def rows(logp, yd):
            logp, state = self._calibrated_logp(logp, use)
            return ops.reliability_rows(logp, on_device(logp, yd), bins=bins, state=state)
        res = ops.reliability_download(self._judge(ds, rows))
        self._refuse_labels("reliability", res["bad_labels"], len(ds), len(self.classes_))
        res["temperature"] = float(self.temperature_) if use else 1.0
        return self._report_calibration(res, use)

    def ranking(self, X, y=None, calibrated=True):
        """Ranking metrics of this fit's predictions on ``X`` (``y``: the labels; None: the dataset's): per class the one-vs-rest
        ROC AUC and the average precision, and their averages over the defined classes, from one ``ops.ranking_rows`` call on the
        device log-probs of ``predict_proba``'s forward passes: ``ops.ranking_download``'s dict -- auc_macro, auc_weighted,
        ap_macro, ap_weighted, classes_scored, auc / ap / support per class (NaN for a class without a positive or a negative
        row), rows, bad_labels, nan_classes -- plus ``classes`` (``classes_``) and ``temperature``.  A temperature changes the
        order of a class's scores ACROSS rows, so a calibrated fit is ranked on its calibrated float32 log-probs
        (``ops.scale_logp`` first) unless ``calibrated=False``; ``temperature`` is then ``temperature_``, else 1.0."""
        self._require_initialized()
        ds = self._as_dataset(X)
        use = self._uses_temperature(calibrated)
        _, on_device = self._labels("ranking", ds, y)

        def rows(logp, yd):
            logp = self._calibrated_values(logp, use)            # in place: the ranks are those of the calibrated log-probs
            return ops.ranking_rows(logp, on_device(logp, yd), per_row=False)
        res = ops.ranking_download(self._judge(ds, rows))
        self._refuse_labels("ranking", res["bad_labels"], len(ds), len(self.classes_))
        res["classes"] = self.classes_
        res["temperature"] = float(self.temperature_) if use else 1.0
        return self._report_calibration(res, use)

    def predict_topk(self, X, k=5, calibrated=True):
        """The ``k`` most probable classes of every sample of ``X`` and their probabilities: ``(labels [N, k] from classes_, proba
        float64 [N, k])``, most probable first, from one ``ops.topk_rows`` call on the device log-probs of ``predict_proba``'s
        forward passes (k in 1..min(classes, 64)).  The order is the arg-max's -- equal log-probs by ascending class -- so
        ``labels[:, 0]`` is ``predict(X)``; the probabilities are softmax(z / T) in fp64, ``temperature_`` for a calibrated fit
        unless ``calibrated=False``, else T = 1."""
        self._require_initialized()
        k = ops._int_in("predict_topk", "k", k, 1, min(len(self.classes_), ops._lib.TOPK_MAX))
        ds = self._as_dataset(X)
        use = self._uses_temperature(calibrated)

        def rows(logp, yd):
            logp, state = self._calibrated_logp(logp, use)
            return ops.topk_rows(logp, k, state=state)
        idx, prob = ops.topk_download(self._judge(ds, rows))
        return self.classes_[idx], prob

    def error_analysis(self, X, y=None, pairs=20, top_k=None, matrix=True, calibrated=True):
        """Which classes this fit gets wrong on ``X`` (``y``: the labels; None: the dataset's) and what it takes them for, formed
        on the device from the log-probs of ``predict_proba``'s forward passes (``ops.error_analysis_rows``: the arg-max and class
        counts, the confusion matrix, its most-confused pairs, the top-k lists) and downloaded in one copy.  A dict:
        ``classes`` (``classes_``); ``confusion`` int64 [V, V], rows true and columns predicted -- None with ``matrix=False``,
        and then the V x V counts never leave the device; ``report`` {precision, recall, f1, support, predicted} per class and
        ``macro`` {precision, recall, f1} (``metrics.class_report``: zero_division = 0, means over all V classes); ``accuracy``;
        ``pairs``: up to ``pairs`` (1..64) tuples (true label, predicted label, count) over the off-diagonal cells, largest
        count first, ties by true then predicted class; ``topk``: ``predict_topk(X, top_k, calibrated)``'s pair from the same
        forward passes, None without ``top_k``; ``rows``: the number of samples."""
        self._require_initialized()
        V = len(self.classes_)
        M = ops._int_in("error_analysis", "pairs", pairs, 1, ops._lib.PAIRS_MAX)
        k = 0 if top_k is None else ops._int_in("error_analysis", "top_k", top_k, 1, min(V, ops._lib.TOPK_MAX))
        if V > ops._lib.CONFUSION_MAX_V:
            raise ValueError(f"error_analysis: {V} classes, the confusion matrix is formed for at most {ops._lib.CONFUSION_MAX_V}")
        ds = self._as_dataset(X)
        use = self._uses_temperature(calibrated)
        _, on_device = self._labels("error_analysis", ds, y)

        def rows(logp, yd):
            logp, state = self._calibrated_logp(logp, use)
            buf = ops.error_analysis_buffers(logp.shape[0], logp.shape[1], k, M, logp.device)
            return ops.error_analysis_rows(logp, on_device(logp, yd), buf, state=state)
        got = ops.error_analysis_download(self._judge(ds, rows), matrix=bool(matrix), topk=k > 0)
        counts = got["counts"]
        V = (counts.size - 1) // 3                           # the columns of the log-probs
        self._refuse_labels("error_analysis", counts[3 * V], len(ds), V)
        report, macro = metrics.class_report(counts[:V], counts[V:2 * V], counts[2 * V:3 * V])
        return self._report_calibration(
            {"classes": self.classes_, "confusion": got["confusion"], "report": report, "macro": macro,
             "accuracy": float(counts[2 * V:3 * V].sum() / len(ds)),
             "pairs": [(self.classes_[t], self.classes_[p], int(c)) for t, p, c in got["pairs"] if c > 0],
             "topk": (self.classes_[got["topk_idx"]], got["topk_prob"]) if k else None, "rows": len(ds)}, use)

    def _interval_request(self, what, scoring, replicates, level, seed):
        """The checked arguments of ``score_interval`` / ``compare``: ``(names, top_k, replicates, level, seed)``."""
        V = len(self.classes_)
        if V > ops._lib.CONFUSION_MAX_V:
            raise ValueError(f"{what}: {V} classes, the bootstrap counts at most {ops._lib.CONFUSION_MAX_V}")
        if scoring is None:                                  # everything that has an interval (top_k_accuracy: k = 2, needs V > 2)
            names = [n for n in metrics.BOOT_COLUMNS if n != "top_k_accuracy" or V > 2] + [v[0] for v in metrics.BOOT_VALUES]
        else:
            names = [scoring] if isinstance(scoring, str) else list(scoring) if isinstance(scoring, (list, tuple)) else []
            if not names or not all(isinstance(n, str) for n in names) or len(set(names)) != len(names):
                raise ValueError(f"{what}: scoring={scoring!r}, expected None, a name or a list of distinct names")
        ks = set()
        for n in names:
            if n in metrics.CALIBRATION[:2] or n.startswith("neg_ece"):
                raise ValueError(f"{what}: {n} has no bootstrap interval here: ECE and MCE are no means over rows, a replicate would need "
                                 "its own bin sums; neg_brier, neg_log_loss and confidence have one")
            found = metrics.bootstrap_metric_of(n)
            if found is None:
                raise ValueError(f"{what}: {n!r} has no bootstrap interval; known: {metrics.BOOT_COLUMNS[:-1]}, top_k_accuracy, "
                                 f"top<k>_accuracy, {tuple(v[0] for v in metrics.BOOT_VALUES)}")
            if found[2] is not None:
                if not 1 <= found[2] < V:
                    raise ValueError(f"{what}: {n}: k={found[2]} must lie in [1, {V}) for {V} classes")
                ks.add(found[2])
        if len(ks) > 1:
            raise ValueError(f"{what}: top-k accuracies for k in {sorted(ks)} asked for, one call resamples one k")
        B = ops._int_in(what, "replicates", replicates, 1, ops._lib.BOOT_MAX_REPLICATES)
        seed = ops._int_in(what, "seed", seed, 0, 2 ** 64 - 1)
        return names, (ks.pop() if ks else 0), B, metrics._boot_level(what, level), seed

    def _bootstrap(self, what, X, y, names, top_k, B, seed, calibrated):
        """One forward pass over ``X``, then ``ops.score_interval_rows`` and one download: ``(point {name: full-sample score},
        replicates float64 [B, len(names)], rows)``."""
        ds = self._as_dataset(X)
        use = self._uses_temperature(calibrated)
        labels, on_device = self._labels(what, ds, y)

        def rows(logp, yd):
            logp, state = self._calibrated_logp(logp, use)
            buf = ops.score_interval_buffers(logp.shape[0], logp.shape[1], B, logp.device)
            return ops.score_interval_rows(logp, on_device(logp, yd), buf, top_k=top_k, seed=seed, state=state)
        got = ops.score_interval_download(self._judge(ds, rows))
        counts = got["counts"]
        V = (counts.size - 1) // 3                           # the columns of the log-probs
        self._refuse_labels(what, counts[3 * V], len(ds), V)
        y_true = np.asarray(labels).astype(np.int64)
        where = {n: metrics.bootstrap_metric_of(n) for n in names}
        counted = [n for n in names if where[n][0] < len(metrics.BOOT_COLUMNS)]
        point = metrics.scores_from_rows(counted, y_true, got["pred"], None, got["rank"], counts, V)
        table = metrics.reliability_from_table(got["table"])
        for name, column, sign in metrics.BOOT_VALUES:       # the reliability table's means: confidence, brier, nll
            if name in where:
                point[name] = sign * table[("confidence", "brier", "nll")[column]]
        reps = np.stack([where[n][1] * got["stats"][:, where[n][0]] for n in names], axis=1)
        return point, reps, len(ds)

    def score_interval(self, X, y=None, scoring=None, replicates=1000, level=0.95, seed=0, calibrated=True, return_replicates=False):
        """Percentile bootstrap confidence intervals of this fit's scores on ``X`` (``y``: the labels; None: the dataset's), drawn
        on the device: one forward pass, ``ops.score_rows``, ``ops.reliability_rows`` (at ``temperature_`` for a calibrated fit
        unless ``calibrated=False``), then ``replicates`` resamples of the per-row results (``ops.bootstrap_scores``) and ONE
        download.  ``scoring``: a name or a list of names among accuracy, precision / recall / f1 _macro and _weighted,
        balanced_accuracy, ``top_k_accuracy`` (k = 2) or ``top<k>_accuracy`` (one k per call), ``neg_log_loss``, ``neg_brier`` and
        ``confidence`` (the mean top-class probability); None: all of them.  ``neg_ece`` / ``neg_mce`` are rejected: they are no
        means over rows.  Returns {name: {point, mean, std, lower, upper, n_nan}} plus ``replicates``, ``level``, ``seed`` and
        ``rows``: ``point`` is the full-sample score from the existing paths (``metrics.scores_from_rows``, the reliability
        table); mean, std (ddof = 1) and the ``level`` percentile bounds are ``metrics.bootstrap_intervals`` of the replicates.
        A replicate scores the classes present IN IT, as sklearn would score that resample.  ``neg_log_loss`` here is minus the
        mean of ``reliability_rows``' fp64 nll -- the UNCLIPPED fp64 log-loss of softmax(z / T), not sklearn's float32-clipped
        one that the history's ``neg_log_loss`` restates; its ``point`` is formed the same way.  The resamples depend on
        ``(seed, len(X))`` alone.  ``return_replicates=True`` adds ``names`` and ``replicate_scores`` float64 [replicates,
        len(names)].  Raises ValueError when a label lies outside the classes."""
        self._require_initialized()
        names, top_k, B, level, seed = self._interval_request("score_interval", scoring, replicates, level, seed)
        point, reps, n = self._bootstrap("score_interval", X, y, names, top_k, B, seed, calibrated)
        summary = metrics.bootstrap_intervals(reps, names, level)
        out = {name: dict(point=float(point[name]), **summary[name]) for name in names}
        out.update(replicates=B, level=level, seed=seed, rows=n)
        if return_replicates:
            out.update(names=names, replicate_scores=reps)
        return self._report_calibration(out, self._uses_temperature(calibrated))

    def compare(self, other, X, y=None, scoring=None, replicates=1000, level=0.95, seed=0, calibrated=True, return_replicates=False):
        """The paired bootstrap of this fit against ``other`` on ``X``: both fits are scored as ``score_interval`` does, with ONE
        seed -- so replicate b holds the same rows for both -- and the replicates of ``self - other`` are summarised
        (``metrics.bootstrap_difference``).  Returns {name: {point, mean, std, lower, upper, n_nan, p_not_better}} plus
        ``replicates``, ``level``, ``seed`` and ``rows``: ``point`` is the difference of the full-sample scores,
        ``p_not_better`` the share of replicates in which ``self`` does not beat ``other`` (every name is a score: greater is
        better).  ``return_replicates=True`` adds ``names`` and ``replicate_scores`` (of the difference).  Raises ValueError when
        the two fits' ``classes_`` differ."""
        if not self.initialized_ or not getattr(other, "initialized_", False):
            raise RuntimeError("compare: both NeuralNetClassifier instances must be initialized.")
        if not np.array_equal(np.asarray(self.classes_), np.asarray(other.classes_)):
            raise ValueError(f"compare: the two fits have different classes_ ({len(self.classes_)} and {len(other.classes_)} classes): "
                             "their scores are not comparable")
        names, top_k, B, level, seed = self._interval_request("compare", scoring, replicates, level, seed)
        point_a, reps_a, n = self._bootstrap("compare", X, y, names, top_k, B, seed, calibrated)
        point_b, reps_b, _ = other._bootstrap("compare", X, y, names, top_k, B, seed, calibrated)
        summary = metrics.bootstrap_difference(reps_a, reps_b, names, level)
        out = {name: dict(point=float(point_a[name] - point_b[name]), **summary[name]) for name in names}
        out.update(replicates=B, level=level, seed=seed, rows=n)
        if return_replicates:
            out.update(names=names, replicate_scores=reps_a - reps_b)
        return out

    def score(self, X, y=None):
        ds = self._as_dataset(X)
        return float((self.predict(ds) == (ds.y if y is None else np.asarray(y))).mean())

    # ------------------------------------------------------ conformal sets
    def _conformal_calibrate(self, logp, yd, opts, calibrated):
        """Scores at the calibration draw, then the threshold, on the current stream: ``(device state float64 [4], whether the
        temperature was used)``.  No host wait."""
        use = self._uses_temperature(calibrated)
        logp = logp if logp.dtype == torch.float32 else logp.float()     # (a fit hands its valid split's log-probs over directly)
        logp, cal = self._calibrated_logp(logp, use)
        buf = ops.conformal_buffers(logp.shape[0], logp.shape[1], logp.device, sets=False)
        ops.conformal_rows(logp, yd.contiguous(), buf, method=opts["method"], lam=opts["lam"], k_reg=opts["k_reg"],
                           randomized=opts["randomized"], seed=opts["seed"], draw=CONFORMAL_DRAW_CALIBRATE, state=cal)
        state = torch.empty(4, dtype=torch.float64, device=logp.device)
        return ops.conformal_quantile(buf, opts["alpha"], state=state), use

    def _set_conformal(self, opts, state=None, calibrated=False, labels=None, where="the calibration data", info=None):
        """``conformal_`` -- the options plus ``calibrated``, ``qhat``, ``n``, ``k`` and ``excluded`` -- and the device state
        ``predict_set`` reads its threshold from; None removes them.  ``state``: ``ops.conformal_quantile``'s (one download of
        its four doubles, which waits for the launches); ``info``: a ``conformal_`` read back from a checkpoint instead (qhat
        goes back to the device).  Labels outside the classes raise, as in ``_set_calibration``."""
        if opts is None:
            for k in ("conformal_", "_conf_state"):
                self.__dict__.pop(k, None)
            return
        if info is None:
            if labels is not None:
                bad = int(((np.asarray(labels) < 0) | (np.asarray(labels) >= len(self.classes_))).sum())
                if bad:
                    raise ValueError(f"conformalizing on {where}: {bad} of {len(labels)} labels lie outside the classes of the log-probs")
            h = state.cpu().numpy()
            info = {**opts, "calibrated": bool(calibrated), "qhat": float(h[0]), "n": int(h[1]), "k": int(h[2]), "excluded": int(h[3])}
            if math.isinf(info["qhat"]):
                warnings.warn(f"conformal: {info['n']} calibration rows are too few for alpha={info['alpha']}: the threshold is infinite "
                              f"and every set holds every class; at least {conformal_least_rows(info['alpha'])} rows are needed",
                              RuntimeWarning, stacklevel=3)
        else:
            dev = self.module_._arena.device if hasattr(self.module_, "_arena") else torch.device(self.device)
            state = torch.tensor([float(info["qhat"]), float(info["n"]), float(info["k"]), float(info["excluded"])],
                                 dtype=torch.float64).to(dev)
        self._conf_state, self.conformal_ = state, dict(info)

    def conformalize(self, X, y=None, alpha=0.1, method="aps", randomized=True, lam=0.0, k_reg=0, seed=0, calibrated=True):
        """Take the threshold of split conformal prediction sets on ``X`` (``y``: the labels; None: the dataset's) -- rows the fit
        has not seen, for the guarantee to hold: with exchangeable rows, ``predict_set`` then covers the true class with
        probability at least 1 - alpha (and, randomised, at most 1 - alpha + 1 / (n + 1)).  One forward pass,
        ``ops.conformal_rows`` at draw 0 and ``ops.conformal_quantile``, all on the device; only the four doubles of the state
        come to the host.  ``method`` "lac": s = 1 - p of the class (the smallest sets on average, may be empty); "aps": the
        probability mass in front of the class plus u times its own (adaptive: larger sets where the model is lost); ``lam`` > 0
        with ``k_reg`` adds RAPS' penalty lam max(0, rank - k_reg), which shortens the tails.  ``randomized``: u is one draw
        per row of the counter-based generator under ``seed``; False: u = 1 (conservative, sets never empty for APS).
        ``calibrated``: the probabilities are softmax(z / T) with ``temperature_`` when the fit has one.  Sets ``conformal_``
        (the options, ``calibrated``, ``qhat``, ``n``, ``k``, ``excluded``: rows left out for a NaN) and returns self.  Fewer than
        about (1 - alpha) / alpha rows give an infinite threshold: kept and reported, with a warning."""
        self._require_initialized()
        opts = conformal_options({"alpha": alpha, "method": method, "randomized": randomized, "lam": lam, "k_reg": k_reg, "seed": seed})
        ds = self._as_dataset(X)
        labels, on_device = self._labels("conformalize", ds, y, check=True)
        state, use = self._judge(ds, lambda logp, yd: self._conformal_calibrate(logp, on_device(logp, yd), opts, calibrated))
        self._set_conformal(opts, state, use, labels=labels)
        return self

    def _conformal_rows(self, what, logp, yd, sets):
        """``ops.conformal_rows`` at the prediction draw under ``conformal_``'s options and the device threshold (a bias calibration
        is applied to ``logp`` in place first: what the caller reads of ``logp`` afterwards is calibrated too)."""
        c = self.conformal_
        logp, state = self._calibrated_logp(logp, self._uses_temperature(c["calibrated"]))
        buf = ops.conformal_buffers(logp.shape[0], logp.shape[1], logp.device, sets=sets)
        return ops.conformal_rows(logp, yd, buf, method=c["method"], lam=c["lam"], k_reg=c["k_reg"], randomized=c["randomized"],
                                  seed=c["seed"], draw=CONFORMAL_DRAW_PREDICT, state=state, qhat=self._conf_state)

    def predict_set(self, X, return_mask=False):
        """The conformal prediction set of every sample of ``X`` under ``conformal_``'s options and threshold (draw 1: a row's u
        is independent of the calibration draws): ``{"sets": ..., "sizes": int array [N]}``.  ``sets``: a list of N label
        arrays (from ``classes_``), most probable first -- every score here grows with the rank, so a set is the first ``size``
        classes of the row's order; the order comes from ``ops.topk_rows`` on the same forward passes, and the members beyond
        rank 64 follow by ascending class -- or, with ``return_mask=True``, a bool [N, V] mask.  A set may be empty (LAC, or
        APS without randomisation when the top probability exceeds the threshold); a row with a NaN gets an empty set.  The
        [N, V] log-probs stay on the device: the set words, the sizes and (for the lists) the top indices come over."""
        self._require_initialized()
        if getattr(self, "conformal_", None) is None:
            raise RuntimeError("predict_set: this estimator has no threshold yet: fit it with the conformal option or call conformalize(X, y)")
        ds = self._as_dataset(X)
        V = len(self.classes_)
        k = min(V, ops._lib.TOPK_MAX)

        def rows(logp, yd):
            buf = self._conformal_rows("predict_set", logp, None, True)
            top = None if return_mask else ops.topk_rows(logp, k)[0]
            return buf, top
        buf, top = self._judge(ds, rows)
        got = ops.conformal_download(buf, rows=True, sets=True)
        sizes = got["rows"][:, 0].astype(np.int64)
        mask = np.unpackbits(got["sets"].view(np.uint8), axis=1, bitorder="little")[:, :V].astype(bool)
        if return_mask:
            return {"sets": mask, "sizes": sizes}
        top = top.cpu().numpy()
        sets = []
        for i in range(len(ds)):
            head = top[i, :min(int(sizes[i]), k)]
            if sizes[i] > k:                                 # the members past rank 64, by ascending class
                rest = mask[i].copy()
                rest[head] = False
                head = np.concatenate([head, np.flatnonzero(rest)])
            sets.append(self.classes_[head])
        return {"sets": sets, "sizes": sizes}

    def coverage(self, X, y=None, min_support=5):
        """What the sets of ``predict_set`` achieve on labelled data ``X`` (``y``: the labels; None: the dataset's), reduced on the
        device (``ops.conformal_summary``) and downloaded in one copy: ``metrics.conformal_report``'s dict -- coverage,
        mean_size, median_size, empty_rate, singleton_rate, size_hist, per class support / class_coverage / class_mean_size
        (NaN for a class without rows), worst_class_coverage over the classes with at least ``min_support`` rows, rows,
        excluded -- plus ``qhat``, ``calibration_rows``, ``k``, ``alpha`` and ``classes``.  The per-class table shows whether
        one threshold serves every class."""
        self._require_initialized()
        if getattr(self, "conformal_", None) is None:
            raise RuntimeError("coverage: this estimator has no threshold yet: fit it with the conformal option or call conformalize(X, y)")
        ds = self._as_dataset(X)
        _, on_device = self._labels("coverage", ds, y, check=True)

        def rows(logp, yd):
            yd = on_device(logp, yd)
            buf = self._conformal_rows("coverage", logp, yd, False)
            ops.conformal_summary(buf, yd)
            return buf
        got = ops.conformal_download(self._judge(ds, rows))
        c = self.conformal_
        res = metrics.conformal_report(got["table"], min_support=min_support)
        res.update(qhat=c["qhat"], calibration_rows=c["n"], k=c["k"], alpha=c["alpha"], classes=self.classes_)
        return res

    # ------------------------------------------------ selective prediction
    def _selective_pass(self, what, ds, labels_on_device, score, calibrated, risks=(), coverages=()):
        """One forward pass, ``ops.selective_rows`` and ``ops.selective_counts`` on the device log-probs, ONE download (32 bytes a
        row): ``(ops.selective_download's dict, whether the temperature was used, the device)``."""
        use = self._uses_temperature(calibrated)

        def rows(logp, yd):
            logp, state = self._calibrated_logp(logp, use)
            buf = ops.selective_rows(logp, labels_on_device(logp, yd), score=score, state=state)
            ops.selective_counts(buf, risks, coverages)
            return buf
        buf = self._judge(ds, rows)
        return ops.selective_download(buf), use, buf["flat"].device

    def risk_coverage(self, X, y=None, score="max_prob", calibrated=True, risks=(0.01, 0.05, 0.1), coverages=(0.5, 0.8, 0.9, 1.0), curve=True):
        """Whether this fit's confidence ranks its own errors on ``X`` (``y``: the labels; None: the dataset's): if it may decline
        to answer below a confidence threshold, how wrong is it on what it does answer.  One forward pass, ``ops.selective_rows``
        and ``ops.selective_counts`` on the device log-probs and one download of 32 bytes a row; ``metrics.selective_report``'s
        dict -- rows, errors, accuracy, excluded_labels, excluded_nan, risk_sum, aurc (the area under the risk-coverage curve,
        Geifman & El-Yaniv), aurc_oracle, e_aurc, coverage_at_risk (per level of ``risks``, up to 8), risk_at_coverage (per level
        of ``coverages``, up to 8), curve (the distinct thresholds in descending order with accepted, wrong, coverage, risk; None
        with ``curve=False``) -- plus ``score``, ``classes`` and ``temperature``.  ``score``: the confidence, "max_prob" (the
        top-class probability), "margin" (the gap to the runner-up) or "neg_entropy".  The probabilities are softmax(z / T) with
        ``temperature_`` for a calibrated fit unless ``calibrated=False``; a temperature changes the order of the confidences
        ACROSS rows, so it changes the curve.  The levels are empirical: they carry no guarantee (``fit_rejection`` gives one).
        Raises ValueError when a label lies outside the classes."""
        self._require_initialized()
        if score not in SELECTIVE_SCORES:
            raise ValueError(f"risk_coverage: score={score!r}, expected one of {SELECTIVE_SCORES}")
        risks, coverages = ops._selective_levels("risk_coverage", "risks", risks), ops._selective_levels("risk_coverage", "coverages", coverages)
        ds = self._as_dataset(X)
        _, on_device = self._labels("risk_coverage", ds, y, check=True)
        got, use, _ = self._selective_pass("risk_coverage", ds, on_device, score, calibrated, risks, coverages)
        res = metrics.selective_report(got["kappa"], got["rows"], got["counts"], got["table"], risks, coverages, curve=bool(curve))
        res.update(score=score, classes=self.classes_, temperature=float(self.temperature_) if use else 1.0)
        return self._report_calibration(res, use)

    def _set_rejection(self, info, device=None):
        """``rejection_`` and the device state ``predict_selective`` reads its threshold from (float64 [4]: tau, n, accepted,
        excluded); None removes them.  ``device``: where the state goes (default: where the fit's weights are)."""
        if info is None:
            for k in ("rejection_", "_rej_state"):
                self.__dict__.pop(k, None)
            return
        if device is None:
            device = self.module_._arena.device if hasattr(self.module_, "_arena") else torch.device(self.device)
        self._rej_state = torch.tensor([float(info["threshold"]), float(info["n"]), float(info["accepted"]), float(info["excluded"])],
                                       dtype=torch.float64).to(device)
        self.rejection_ = dict(info)

    def fit_rejection(self, X, y=None, target_risk=0.05, delta=0.05, score="max_prob", calibrated=True):
        """Turn a target error rate into a rejection threshold on ``X`` (``y``: the labels; None: the dataset's) -- rows the fit
        NEVER SAW, neither in training nor for early stopping, the temperature or a conformal threshold, and drawn like the rows
        ``predict_selective`` will meet: only then does the guarantee hold.  One forward pass, the risk-coverage curve on the
        device (``risk_coverage``'s), then ``metrics.guaranteed_threshold``: with ``delta`` the SGR search of Geifman and El-Yaniv
        (2017), after which the selective risk on new rows exceeds ``target_risk`` with probability at most ``delta`` over the
        draw of ``X``; ``delta=None``: the ``empirical`` rule, the largest coverage whose empirical risk is at most the target,
        which carries no guarantee.  Sets ``rejection_`` = {score, rule, target_risk, delta, threshold, bound, accepted, wrong,
        coverage, risk, n, excluded, calibrated}; the threshold is one of the device's own confidences bit for bit and goes
        back into a device state that ``predict_selective`` reads.  Returns self.

        The search probes about log2(n) thresholds and the bound is not monotone in the number of accepted rows, so at small n
        it can miss a threshold that exists: on the population of tests/test_selective_cpu.py (confidence uniform, P[wrong] =
        (1 - confidence)^2), target 0.05, delta 0.05, 137 of 400 draws of n = 1000 rows found nothing (about a third: 146 of 400
        under another seed) and none of 400 draws of n = 4000.
        When nothing qualifies the threshold is +inf and nothing is accepted: kept and reported, with a RuntimeWarning."""
        self._require_initialized()
        if score not in SELECTIVE_SCORES:
            raise ValueError(f"fit_rejection: score={score!r}, expected one of {SELECTIVE_SCORES}")
        ds = self._as_dataset(X)
        _, on_device = self._labels("fit_rejection", ds, y, check=True)
        empty = {"threshold": [], "accepted": [], "wrong": [], "coverage": [], "risk": []}
        metrics.guaranteed_threshold(empty, target_risk, delta)                  # the options' own checks, before the forward passes
        got, use, device = self._selective_pass("fit_rejection", ds, on_device, score, calibrated)
        rep = metrics.selective_report(got["kappa"], got["rows"], got["counts"], got["table"])
        pick = metrics.guaranteed_threshold(rep["curve"], target_risk, delta)
        info = {"score": score, "rule": "empirical" if delta is None else "sgr", "target_risk": float(target_risk),
                "delta": None if delta is None else float(delta), "threshold": float("inf"), "bound": None, "accepted": 0, "wrong": 0,
                "coverage": 0.0, "risk": float("nan"), "n": rep["rows"], "excluded": rep["excluded_labels"] + rep["excluded_nan"],
                "calibrated": bool(use)}
        if pick is None:
            warnings.warn(f"fit_rejection: no threshold on these {rep['rows']} rows holds the selective risk at {float(target_risk):g}"
                          + ("" if delta is None else f" with confidence {1.0 - float(delta):g}")
                          + ": the threshold is infinite and nothing is accepted; more rows, a larger target or a larger delta may find one",
                          RuntimeWarning, stacklevel=2)
        else:
            info.update({k: pick[k] for k in ("threshold", "bound", "accepted", "wrong", "coverage", "risk")})
        self._set_rejection(info, device)
        return self

    def predict_selective(self, X):
        """Predict with the reject option at ``rejection_``'s threshold: ``{"labels": from classes_ [N], "accepted": bool [N],
        "confidence": float64 [N]}`` -- a row is accepted when its confidence (``rejection_["score"]``, at the temperature the
        threshold was taken at) is at least the threshold, compared on the device against the device state; a row that holds a
        NaN has a NaN confidence and is rejected.  ``labels`` are ``predict``'s whether accepted or not.  One forward pass, one
        download of 24 bytes a row."""
        self._require_initialized()
        if getattr(self, "rejection_", None) is None:
            raise RuntimeError("predict_selective: this estimator has no rejection threshold yet: call fit_rejection(X, y) first")
        r = self.rejection_
        use = self._uses_temperature(r["calibrated"])

        def rows(logp, yd):
            logp, state = self._calibrated_logp(logp, use)
            return ops.selective_rows(logp, None, score=r["score"], state=state, tau=self._rej_state)
        got = ops.selective_download(self._judge(self._as_dataset(X), rows), counts=False)
        return {"labels": self.classes_[got["rows"][:, 0]], "accepted": got["rows"][:, 2] != 0, "confidence": got["kappa"]}

    # ------------------------------------------------------------ label audit
    def label_issues(self, X, y=None, calibrated=True, rank_by="normalized_margin", pairs=20, per_row=False):
        """Which labels of ``X`` (``y``: the labels; None: the dataset's) are probably wrong, by confident learning (Northcutt, Jiang
        and Chuang 2021): a row is CONFIDENTLY class c when its probability of c reaches t_c, the mean self-confidence of the rows
        labelled c; a row confidently another class than its given one is a label issue, and that class is the suggestion.  One
        forward pass, ``ops.label_audit_rows`` on the device log-probs and one download; ``metrics.label_audit_report``'s dict --
        issues {row, given, suggested, self_confidence, margin} most suspicious first under ``rank_by`` ("normalized_margin" |
        "self_confidence"), joint, calibrated_joint, noise_rate, per_class {support, threshold, issues, confident_other, noise},
        pairs (given, suggested, count: up to ``pairs`` likely label swaps, 1..64), rows, bad_labels, nan_rows, unconfident,
        argmax_disagrees -- with ``given``, ``suggested`` and the pairs as ``classes_`` entries, plus ``classes`` and
        ``temperature``.  ``per_row=True`` adds ``per_row``: k, code, flags, pred int32 [N], s, m, other, p_pred float64 [N].  The
        probabilities are softmax(z / T) with ``temperature_`` for a calibrated fit unless ``calibrated=False``.

        The audit judges labels only on log-probs of rows the model was NOT fitted on: a fit has memorised its own training
        rows, so use ``slnlp.cross_fit`` / ``slnlp.OutOfFold`` for a training set.  And it is meaningful for the two RNN models
        only: the reference Transformer feeds the gold label to its decoder, so its log-probs of a row already depend on that
        row's label -- for it this is a statement about the log-probs, not about the labels.  Raises ValueError when a label lies
        outside the classes."""
        self._require_initialized()
        if rank_by not in metrics.LABEL_RANKINGS:
            raise ValueError(f"label_issues: rank_by={rank_by!r}, expected one of {metrics.LABEL_RANKINGS}")
        M = ops._int_in("label_issues", "pairs", pairs, 1, ops._lib.PAIRS_MAX)
        if len(self.classes_) > ops._lib.CONFUSION_MAX_V:
            raise ValueError(f"label_issues: {len(self.classes_)} classes, the confident joint is formed for at most {ops._lib.CONFUSION_MAX_V}")
        ds = self._as_dataset(X)
        use = self._uses_temperature(calibrated)
        labels, on_device = self._labels("label_issues", ds, y)

        def rows(logp, yd):
            logp, state = self._calibrated_logp(logp, use)
            return ops.label_audit_rows(logp, on_device(logp, yd), state=state, pairs=M)
        got = ops.label_audit_download(self._judge(ds, rows), per_row=bool(per_row))
        self._refuse_labels("label_issues", got["head"][1], len(ds), len(self.classes_))
        res = metrics.label_audit_report(got, labels, rank_by=rank_by)
        res["issues"]["given"] = self.classes_[res["issues"]["given"]]
        res["issues"]["suggested"] = self.classes_[res["issues"]["suggested"]]
        res["pairs"] = [(self.classes_[g], self.classes_[c], cnt) for g, c, cnt in res["pairs"]]
        res.update(classes=self.classes_, temperature=float(self.temperature_) if use else 1.0)
        self._report_calibration(res, use)
        if per_row:
            res["per_row"] = {q: got[q] for q in ("k", "code", "flags", "pred", "s", "m", "other", "p_pred")}
        return res

    # ----------------------------------------------------------- attribution
    def attribute(self, X, y=None, by="frame", mode="mask", width=1, stride=1, bins=8, substitutions=None, unit_names=None,
                  target="label", calibrated=True, per_variant=False, max_variants=65536):
        """What in the input this fit's predictions on ``X`` rest on, by occlusion: hide one unit of a row, run the forward passes
        again and measure how far the log-probability of the class falls.  ``by`` "frame": the units are the frames, one at a
        time (``width`` 1; ``stride`` > 1 takes every stride-th); "window": windows of ``width`` frames every ``stride``; ``mode``
        "mask" replaces the window's tokens by ``<unk>``, "drop" deletes them and closes the row up (a window over the whole row
        is masked).  ``by`` "field": the units are the phonological fields a token is composed from; ``substitutions`` int64
        [len(vocab_X), F] (``slnlp.ingest.field_substitutions``) maps every token to itself with one field nulled.  ``target``:
        the class whose log-probability is followed, "label" (``y``, or the dataset's) or "pred" (the base row's arg-max).

        One base pass, its calibrated log-probs kept on the device; then the rows of ``X`` in chunks of at most
        ``max_variants`` variants: ``ops.occlude_rows`` builds the chunk's inputs ON THE DEVICE, the forward passes take them as
        ``slnlp.data.DeviceRows`` through the same hook every consumer uses, and ``ops.attribution_rows`` reduces each variant row
        against its base row under the same calibration; one ``ops.attribution_summary`` and ONE download -- the M x V variant
        log-probs never leave the device.  Returns ``metrics.attribution_report``'s dict -- per row top_unit, top_drop, min_drop,
        sum_drop, flips, units, base_pred, target, base_logp; per_bin and per_class {mean_drop, mean_kl, flip_rate, count,
        nonfinite} (a bin is the relative position of the window's centre in ``bins`` equal parts of the row, or the field);
        ranking; unit_names; the head's counts -- with ``base_pred`` and ``target`` as indices into ``classes`` (target -1: the row
        has none), plus ``classes``, ``temperature``, ``rows`` and ``by`` / ``mode`` / ``width`` / ``stride`` / ``target_kind``.  ``per_variant=True`` adds ``per_variant``:
        variants int32 [M, 3] = (row, unit, bin), row_start, drop / dp / kl float64 [M], pred and code int32 [M].

        drop = lp_base(c) - lp_variant(c), so a POSITIVE drop says the unit supports class c.  Occlusion measures what THIS model
        uses, not what is in the signal, and ``<unk>`` / the null field are themselves tokens the model has a reaction to.  The
        statement is as asked for the two RNN models only: the reference Transformer feeds the gold label to its decoder, so its
        drops are conditional on that label (every variant carries its row's label).  Raises ValueError when a label lies outside
        the classes (``target="label"``) or when no row has a frame to occlude."""
        self._require_initialized()
        what = "attribute"
        o = attribution_options({"by": by, "mode": mode, "width": width, "stride": stride, "bins": bins, "target": target})
        cap = ops._int_in(what, "max_variants", max_variants, 1, (2 ** 31 - 1) // 3)
        V = len(self.classes_)
        if V > ops._lib.CONFUSION_MAX_V:
            raise ValueError(f"{what}: {V} classes, the table is formed for at most {ops._lib.CONFUSION_MAX_V}")
        ds = self._as_dataset(X)
        S = int(ds.ids.shape[1])
        if o["by"] == "field":
            if substitutions is None:
                raise ValueError(f"{what}: by='field' needs substitutions, the table of slnlp.ingest.field_substitutions")
            sub_host = np.ascontiguousarray(np.asarray(substitutions), dtype=np.int64)
            if sub_host.ndim != 2 or not 1 <= sub_host.shape[1] <= ops._lib.ATTR_MAX_BINS or sub_host.shape[0] < 1:
                raise ValueError(f"{what}: substitutions of shape {sub_host.shape}, expected int64 [vocabulary, F] with F in 1..{ops._lib.ATTR_MAX_BINS}")
            kind = "substitute"
            variants, row_start, n_bins = ops.occlusion_variants(ds.lengths, S, "field", n_fields=int(sub_host.shape[1]))
        else:
            if substitutions is not None:
                raise ValueError(f"{what}: substitutions are read with by='field' only")
            if o["width"] > S or o["stride"] > S:
                raise ValueError(f"{what}: width={o['width']} and stride={o['stride']} must lie in 1..{S}, the rows' padded length")
            sub_host, kind = None, o["mode"]
            variants, row_start, n_bins = ops.occlusion_variants(ds.lengths, S, o["mode"], o["width"], o["stride"], o["bins"])
        if unit_names is not None and len(list(unit_names)) != n_bins:
            raise ValueError(f"{what}: {len(list(unit_names))} unit_names for {n_bins} bins")
        M = int(variants.shape[0])
        if M < 1:
            raise ValueError(f"{what}: no row of X has a frame to occlude")
        if M > (2 ** 31 - 1) // 3:
            raise ValueError(f"{what}: {M} variants, at most {(2 ** 31 - 1) // 3} fit one table")
        use = self._uses_temperature(calibrated)
        _, on_device = self._labels(what, ds, y, check=o["target"] == "label")
        pad, unk = 1, 0                                      # the vocabularies' specials: <unk> 0, <pad> 1 (slnlp/ingest.py)
        if getattr(ds, "vocab_X", None) is not None and hasattr(ds.vocab_X, "stoi"):
            pad, unk = int(ds.vocab_X.stoi["<pad>"]), int(ds.vocab_X.stoi["<unk>"])

        def base_rows(logp, yd):                             # the calibrated base log-probs stay on the device
            logp, state = self._calibrated_logp(logp, use)
            return logp, on_device(logp, yd), state
        base, yd, state = self._judge(ds, base_rows)
        dev = base.device
        with torch.cuda.device(dev):
            Xd, Ld = torch.from_numpy(ds.ids).to(dev), torch.from_numpy(ds.lengths).to(dev)
            sub = None if sub_host is None else torch.from_numpy(sub_host).to(dev)
            buf = ops.attribution_buffers(len(ds), V, variants, row_start, n_bins, dev)
        first = 0                                            # whole rows per chunk (one row alone where it has more variants than the cap)
        while first < len(ds):
            last = first + 1
            while last < len(ds) and int(row_start[last + 1]) - int(row_start[first]) <= cap:
                last += 1
            off, m = int(row_start[first]), int(row_start[last]) - int(row_start[first])
            first = last
            if m == 0:
                continue
            with torch.cuda.device(dev):
                rows = DeviceRows(*ops.occlude_rows(Xd, Ld, yd, buf["variants"][off:off + m], kind, width=o["width"], stride=o["stride"],
                                                    pad=pad, unk=unk, sub=sub))

            def variant_rows(logp, _, off=off):
                logp, st = self._calibrated_logp(logp, use)
                return ops.attribution_rows(base, logp, yd, buf, off, target=o["target"], state=st)
            self._judge(rows, variant_rows)
        with torch.cuda.device(dev):
            ops.attribution_summary(base, yd, buf, target=o["target"], state=state)
            got = ops.attribution_download(buf, per_variant=bool(per_variant))
        self._refuse_labels(what, got["head"][1], M, V)
        res = metrics.attribution_report(got, unit_names)
        res.update(classes=self.classes_, temperature=float(self.temperature_) if use else 1.0, by=o["by"], mode=o["mode"], width=o["width"],
                   stride=o["stride"], target_kind=o["target"], rows=len(ds))
        self._report_calibration(res, use)
        if per_variant:
            res["per_variant"] = {"variants": variants, "row_start": row_start, "drop": got["vals"][:, 0], "dp": got["vals"][:, 1],
                                  "kl": got["vals"][:, 2], "pred": got["ints"][:, 0], "code": got["ints"][:, 1]}
        return res
