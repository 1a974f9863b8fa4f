"""Label-shift adaptation: a fit's predictions under other class priors than the ones it was trained under, on the device.

A classifier trained under the priors pi_s and used under pi_t is corrected exactly by p_t(c | x) ~ p_s(c | x) pi_t(c) / pi_s(c).
Here pi_s is near uniform by construction -- the reference resamples the training set (``balance_dataset``), ``iterator_train__balance``
draws class-balanced epochs -- while the rows a fit is judged and used on follow the glosses' long-tailed natural frequencies.
``PriorShift`` wraps an initialised ``NeuralNetClassifier`` or a ``VotingEnsemble``, estimates pi_t from UNLABELLED rows by the EM of
Saerens, Latinne and Decaestecker (2002) (``ops.fit_priors``: the maximum-likelihood estimate; on calibrated probabilities the
method to beat, Alexandari et al. 2020, so the base's fitted temperature is folded in) and re-weights the base's device log-probs
in place (``ops.shift_logp``) before they reach whatever judges them: the wrapper is a ``slnlp.judge.LogProbJudge``, so
``predict_proba``, ``predict``, ``reliability``, ``ranking``, ``predict_topk``, ``error_analysis``, ``score_interval``, ``compare``,
``conformalize``, ``predict_set``, ``coverage``, ``risk_coverage``, ``fit_rejection``, ``predict_selective``, ``label_issues`` and ``attribute`` all see the adapted
predictions.  No torch arithmetic runs on the device.

"Unlabelled" is honest for the two RNN models only: the reference Transformer feeds the gold label to its decoder (SURVEY.md
section 3.4 quirk 1, reproduced for parity), so its log-probs of a row already depend on that row's label.  The adaptation works on
log-probs and does not care which model formed them; what the estimate means for the Transformer is the caller's judgement."""
import numbers

import numpy as np
import torch
from sklearn.base import BaseEstimator, ClassifierMixin

from . import ops
from .data import TokenDataset
from .ensemble import VotingEnsemble
from .judge import LogProbJudge
from .net import NeuralNetClassifier


def _smoothing(what, smoothing):
    if isinstance(smoothing, bool) or not isinstance(smoothing, numbers.Real) or not 0.0 <= float(smoothing) < float("inf"):
        raise ValueError(f"{what}: smoothing={smoothing!r}, expected a finite number >= 0")
    return float(smoothing)


def normalised_priors(what, values, V, smoothing=0.0):
    """``values`` -- V probabilities or counts, finite and >= 0 -- plus ``smoothing`` on every entry, divided by their sum:
    float64 [V].  Raises ValueError for another length, and one that names the classes that are still zero."""
    smoothing = _smoothing(what, smoothing)
    try:
        v = np.asarray(values, dtype=np.float64)
    except (TypeError, ValueError):
        v = None
    if v is None or v.shape != (V,):
        raise ValueError(f"{what}: expected {V} probabilities or counts, one per class, got "
                         f"{'shape ' + str(tuple(v.shape)) if v is not None else repr(values)}")
    if not (np.isfinite(v).all() and (v >= 0.0).all()):
        raise ValueError(f"{what}: the {V} values must be finite and >= 0")
    v = v + smoothing
    empty = np.flatnonzero(v == 0.0)
    if empty.size:
        raise ValueError(f"{what}: classes {empty.tolist()} have prior 0 (smoothing={smoothing:g}): a class the fit never saw cannot be "
                         "re-weighted; pass smoothing > 0")
    return v / v.sum()


def class_frequencies(y, V, smoothing=0.0):
    """The label frequencies of ``y`` over ``V`` classes with ``smoothing`` added to every count: (count_c + smoothing) / (N + V
    smoothing), float64 [V].  A label outside [0, V) and a class left at zero raise ValueError."""
    y = np.asarray(y)
    if y.ndim != 1 or y.size == 0 or not np.issubdtype(y.dtype, np.integer):
        raise ValueError(f"class_frequencies: y must be a non-empty 1-D integer array, got {y.dtype} {tuple(y.shape)}")
    bad = int(((y < 0) | (y >= V)).sum())
    if bad:
        raise ValueError(f"class_frequencies: {bad} of {y.size} labels lie outside the {V} classes")
    return normalised_priors("class_frequencies", np.bincount(y, minlength=V), V, smoothing)


class PriorShift(LogProbJudge, ClassifierMixin, BaseEstimator):
    """``base``: an initialised ``NeuralNetClassifier`` or a ``VotingEnsemble``.  ``source``: the priors the base was trained under --
    V probabilities or counts (``class_frequencies(y, V, smoothing)`` turns labels into them; ``smoothing`` is added to every entry
    before they are normalised, and every class must end above 0), or a ``TokenDataset``: then the base's mean predicted
    probability on it, taken on the device at the first ``fit`` / ``set_priors`` (Alexandari et al.'s choice: always above 0, and
    the fixed point of the EM on the source data itself).  ``calibrated``: a base that fitted a temperature enters as
    softmax(z / T), one with a ``bias_temperature`` calibration as softmax(beta z + b) -- the probabilities the EM is "hard to beat"
    on (Alexandari et al. 2020); False: at T = 1.  The wrapper has no temperature of its own: ``calibration_`` is None, ``temperature_`` 1.0.

    ``fit(X)`` sets ``priors_`` (the estimated target priors), ``source_priors_``, ``log_ratio_`` (ln of their ratio, what the
    device adds to the log-probs) and ``prior_shift_`` (``ops.priors_download``'s dict); ``set_priors`` installs known priors
    instead.  Before either, every method that needs log-probs raises RuntimeError."""
    calibration_ = None
    temperature_ = 1.0
    predict_nonlinearity = "auto"
    initialized_ = True

    def __init__(self, base, source, calibrated=True, smoothing=0.0):
        if not isinstance(base, (NeuralNetClassifier, VotingEnsemble)):
            raise ValueError(f"PriorShift: base must be a NeuralNetClassifier or a VotingEnsemble, got {type(base).__name__}")
        if not getattr(base, "initialized_", False):
            raise RuntimeError("PriorShift: the base must be initialized.")
        if getattr(base, "classes_", None) is None:
            raise ValueError("PriorShift: the base must have classes_ (a fit sets them)")
        V = len(base.classes_)
        _smoothing("PriorShift", smoothing)
        if not isinstance(source, TokenDataset):
            normalised_priors("PriorShift: source", source, V, smoothing)
        self.base, self.source, self.calibrated, self.smoothing = base, source, bool(calibrated), smoothing
        self.classes_ = base.classes_

    # ------------------------------------------------------------- the base
    def _device(self):
        return VotingEnsemble._device_of(self.base.members[0] if isinstance(self.base, VotingEnsemble) else self.base)

    def _base_logp(self, ds, then):
        """The base's float32 log-probs handed to ``then(logp, y_dev, state)`` as the base's own ``_calibrated_logp`` hands them over:
        ``state`` is its device calibration state, or None: beta = 1 -- a ``bias_temperature`` calibration is then already in the
        log-probs, and an ensemble's members' calibrations always are."""
        def calibrated(logp, yd):
            logp = logp if logp.dtype == torch.float32 else logp.float()
            logp, state = self.base._calibrated_logp(logp, self.base._uses_temperature(self.calibrated))
            return then(logp, yd, state)
        return self.base._forward_logp(ds, calibrated)

    def _source_priors(self):
        """``source_priors_``, formed once: the checked vector, or the base's mean prediction on the source dataset -- table row 0
        of an ``ops.fit_priors`` call with ``max_iter=0``."""
        if getattr(self, "source_priors_", None) is None:
            V = len(self.classes_)
            if isinstance(self.source, TokenDataset):
                start = torch.zeros(V, dtype=torch.float64).to(self._device())
                out = self._base_logp(self.source, lambda logp, yd, state: ops.fit_priors(logp, start, state=state, max_iter=0, tol=0.0))
                got = ops.priors_download(out)
                if got["reason"] == "empty":
                    raise ValueError(f"PriorShift: every one of the {len(self.source)} source rows holds a NaN or has no finite maximum")
                self.source_priors_ = normalised_priors("PriorShift: the mean prediction on source", got["mean_proba"], V, self.smoothing)
            else:
                self.source_priors_ = normalised_priors("PriorShift: source", self.source, V, self.smoothing)
        return self.source_priors_

    def _install(self, log_w_dev, priors, info):
        self._log_w, self.priors_, self.prior_shift_ = log_w_dev, priors, info
        with np.errstate(divide="ignore"):
            self.log_ratio_ = info["log_ratio"] if info is not None else np.log(priors) - np.log(self.source_priors_)
        self.__dict__.pop("conformal_", None)                # a threshold taken under other priors does not carry over
        self.__dict__.pop("_conf_state", None)
        self._set_rejection(None)                            # nor does a rejection threshold
        return self

    # --------------------------------------------------------------- fitting
    def fit(self, X, y=None, max_iter=200, tol=1e-6):
        """Estimate the target priors from the rows of ``X`` by EM on the base's device log-probs; the labels of ``X`` and ``y``
        are never read (the dataset's ``y`` travels to the module because the Transformer's decoder consumes it).  ``max_iter``
        in 0..1024 and ``tol``, the largest change of a prior at which the EM stops; ``prior_shift_["reason"]`` says which ended
        it ("tol" | "cap" | "empty": no usable row, the priors stay the source's).  One forward pass, one queued launch
        sequence, one download."""
        max_iter = ops._int_in("PriorShift.fit", "max_iter", max_iter, 0, ops._lib.PRIOR_MAX_ITER)
        if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not 0.0 <= float(tol) < float("inf"):
            raise ValueError(f"PriorShift.fit: tol={tol!r}, expected a finite number >= 0")
        ds = self._as_dataset(X)
        log_source = torch.from_numpy(np.log(self._source_priors())).to(self._device())
        out = self._base_logp(ds, lambda logp, yd, state: ops.fit_priors(logp, log_source, state=state, max_iter=max_iter, tol=float(tol)))
        info = ops.priors_download(out)
        V = len(self.classes_)
        return self._install(out[2 * V:3 * V], info["priors"], info)

    def set_priors(self, priors):
        """Install known target priors -- V probabilities or counts, finite and >= 0 with a positive sum; a class at 0 gets
        probability 0 -- without any EM; ``prior_shift_`` is None."""
        V = len(self.classes_)
        try:
            p = np.asarray(priors, dtype=np.float64)
        except (TypeError, ValueError):
            p = None
        if p is None or p.shape != (V,) or not (np.isfinite(p).all() and (p >= 0.0).all() and p.sum() > 0.0):
            raise ValueError(f"PriorShift.set_priors: expected {V} finite probabilities or counts >= 0 with a positive sum")
        p = p / p.sum()
        with np.errstate(divide="ignore"):
            log_w = np.log(p) - np.log(self._source_priors())
        return self._install(torch.from_numpy(log_w).to(self._device()), p, None)

    # ------------------------------------------------------------- the hook
    def _forward_logp(self, ds, then):
        """The base's float32 log-probs [len(ds), V] re-weighted in place on the device -- on the base's stream, under its gate --
        and handed to ``then(logp, y_dev)``: the hook every consumer of ``LogProbJudge`` goes through."""
        if getattr(self, "_log_w", None) is None:
            raise RuntimeError("PriorShift: no target priors yet: call fit(X) or set_priors(priors) first")

        def shifted(logp, yd, state):
            ops.shift_logp(logp, self._log_w, state=state, out=logp)
            return then(logp, yd)
        return self._base_logp(ds, shifted)
