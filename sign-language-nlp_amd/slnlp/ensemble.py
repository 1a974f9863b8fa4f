"""Soft-voting ensembles of fitted ``NeuralNetClassifier``s, combined on the device.

``VotingEnsemble`` predicts with several fits at once -- the folds of a cross-validation, the seeds of one configuration: every
member runs its own forward passes (``NeuralNetClassifier._forward_logp``: under its gate, on its stream, with its averaged
weights where it predicts with them), ONE ``ops.ensemble_rows`` launch combines the members' device log-probs, each at its own
temperature, into one set of float32 log-probs, and everything that judges one fit's log-probs -- ``predict_proba``,
``reliability``, ``ranking``, ``predict_topk``, ``error_analysis``, ``score_interval``, ``compare``, ``conformalize``, ``predict_set``,
``coverage``, ``risk_coverage``, ``fit_rejection``, ``predict_selective``, ``label_issues``, ``attribute`` -- then works on the ensemble through the
same ``_forward_logp(ds, then)`` hook: both classes inherit those methods from ``slnlp.judge.LogProbJudge``.  The
same launch gives, per sample, how much the members disagree (``uncertainty``): the entropy of the mixture, the expected entropy
of a member and their difference, the mutual information.  Nothing is averaged on the host and no torch arithmetic runs on the
device."""
import numpy as np
import torch
from sklearn.base import BaseEstimator, ClassifierMixin

from . import _lib, ops
from .judge import LogProbJudge
from .net import NeuralNetClassifier, ScoringWrapper, _CachedPredictor, stream_sync

VOTING = tuple(_lib.VOTING)


class VotingEnsemble(LogProbJudge, ClassifierMixin, BaseEstimator):
    """``members``: 1..32 initialised ``NeuralNetClassifier``s on one device with equal ``classes_``.  ``voting``: "soft", the
    weighted arithmetic mean of the members' probabilities, or "log", their weighted geometric mean renormalised (a product of
    experts).  ``weights``: one finite number > 0 per member (normalised on the way in), None: equal.  ``calibrated``: a member
    that fitted a temperature enters as softmax(z / T_k) -- one with a ``bias_temperature`` calibration as its shifted log-probs,
    softmax(beta_k z + b_k), at beta = 1 (``LogProbJudge._calibrated_logp``); False: every member at T = 1.  The ensemble has no
    temperature of its own: ``calibration_`` is None, and the methods that report one report 1.0."""
    calibration_ = None
    temperature_ = 1.0
    predict_nonlinearity = "auto"
    initialized_ = True

    def __init__(self, members, voting="soft", weights=None, calibrated=True):
        members = list(members) if isinstance(members, (list, tuple)) else None
        if not members or len(members) > _lib.ENSEMBLE_MAX_MEMBERS or not all(isinstance(m, NeuralNetClassifier) for m in members):
            raise ValueError(f"VotingEnsemble: members must be a list of 1..{_lib.ENSEMBLE_MAX_MEMBERS} NeuralNetClassifier instances")
        if not all(getattr(m, "initialized_", False) for m in members):
            raise RuntimeError("VotingEnsemble: every member must be initialized.")
        if not all(getattr(m, "classes_", None) is not None for m in members):
            raise ValueError("VotingEnsemble: every member must have classes_ (a fit sets them; a fit read back with load_params takes "
                             "the classes_ of the fit that wrote the files)")
        if voting not in VOTING:
            raise ValueError(f"VotingEnsemble: voting={voting!r}, expected one of {VOTING}")
        first = members[0]
        for k, m in enumerate(members[1:], 1):
            if not np.array_equal(np.asarray(first.classes_), np.asarray(m.classes_)):
                raise ValueError(f"VotingEnsemble: member {k} and member 0 have different classes_ ({len(m.classes_)} and "
                                 f"{len(first.classes_)} classes): their probabilities are not comparable")
            if self._device_of(m) != self._device_of(first):
                raise ValueError(f"VotingEnsemble: member {k} is on {self._device_of(m)}, member 0 on {self._device_of(first)}: the "
                                 "members' log-probs are combined by one launch on one device")
        if weights is not None:
            weights = [float(w) for w in weights] if isinstance(weights, (list, tuple, np.ndarray)) else None
            if weights is None or len(weights) != len(members) or not all(0.0 < w < float("inf") for w in weights):
                raise ValueError(f"VotingEnsemble: weights must be {len(members)} finite numbers above 0 (or None: equal weights)")
        self.members, self.voting, self.weights, self.calibrated = members, voting, weights, bool(calibrated)
        self.classes_ = first.classes_

    @staticmethod
    def _device_of(net):
        dev = torch.device(net.device)
        return torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev

    def _member_logp(self, member):
        """The ``then`` of a member's forward pass: ``(float32 log-probs, y_dev, calibration state or None)`` as the member's own
        ``_calibrated_logp`` hands them over -- a bias calibration is already in the log-probs, on the member's stream."""
        def keep(logp, yd):
            logp = logp if logp.dtype == torch.float32 else logp.float()
            logp, state = member._calibrated_logp(logp, member._uses_temperature(self.calibrated))
            return logp, yd, state
        return keep

    def _combine(self, ds, then, diagnostics):
        """Every member's float32 log-probs of ``ds`` -- its own ``_forward_logp``: under its gate, on its stream, returned once
        that stream has drained -- then, on the first member's stream and under its gate, ``ops.ensemble_rows`` and
        ``then(out, y_dev, rows)``; returns what ``then`` returns once that stream has drained."""
        got = [m._forward_logp(ds, self._member_logp(m)) for m in self.members]
        first = self.members[0]
        first._gate.enter(not first._fused)
        try:
            first._enter_stream()
            with torch.cuda.stream(first._stream), torch.no_grad():
                out, rows = ops.ensemble_rows([g[0] for g in got], states=[g[2] for g in got], weights=self.weights, voting=self.voting,
                                              diagnostics=diagnostics)
                res = then(out, got[0][1], rows)
            stream_sync(first._stream)
        finally:
            first._gate.leave(not first._fused)
        return res

    def _forward_logp(self, ds, then):
        """The ensemble's float32 log-probs [len(ds), V] on the device, handed to ``then(logp, y_dev)``: the hook every
        log-prob consumer of ``NeuralNetClassifier`` goes through."""
        return self._combine(ds, lambda out, yd, rows: then(out, yd), False)

    # the log-prob consumers are LogProbJudge's: they read ``self._forward_logp``, ``classes_``, ``calibration_`` (None here: T = 1);
    # the conformal threshold is the ensemble's own (``conformal_``), taken by ``conformalize``; so is the rejection threshold
    # (``rejection_``, ``fit_rejection``)

    def uncertainty(self, X, per_row=False):
        """How much the members disagree on ``X``: ``metrics.uncertainty_summary`` of ``ops.ensemble_rows``' per-row terms --
        {total_entropy, expected_entropy, mutual_information, disagreement_rate, mean_disagreement, rows, nan_rows}, the means
        over the samples; ``per_row=True`` adds ``per_row``, float64 [N, 4] = (total entropy, expected member entropy, mutual
        information, number of members whose arg-max is not the ensemble's) per sample.  One download, of the rows."""
        return ops.ensemble_download(self._combine(self._as_dataset(X), lambda out, yd, rows: (out, rows), True), per_row=bool(per_row))

    def member_scores(self, X, scoring):
        """The point scores of every member and of the ensemble on ``X`` through the existing scoring path (``ScoringWrapper`` on
        each estimator's ``predict_proba``, a member's at its own temperature):
        {"ensemble": {name: score}, "members": [{name: score}, ...]}; ``scoring``: a name or a list of names."""
        ds = self._as_dataset(X)
        names = [scoring] if isinstance(scoring, str) else list(scoring)
        labels = np.arange(len(self.classes_))

        def one(est):                                        # one forward pass per estimator, whatever the number of names
            cached = _CachedPredictor(est.predict_proba(ds), est.classes_)
            return {n: float(ScoringWrapper(n, labels)(cached, ds, ds.y)) for n in names}
        return {"ensemble": one(self), "members": [one(m) for m in self.members]}
