"""Out-of-fold log-probs of a whole data set, assembled on the device: ``OutOfFold`` and ``cross_fit``.

Every diagnostic of ``slnlp.judge.LogProbJudge`` needs log-probs of rows the model has not been fitted on; a fit has memorised its
own training rows and the held-out test split is a few hundred rows.  Cross-fitting is the standard answer: cv fits, each
predicting the fold it did not see, assembled in row order.  ``OutOfFold`` holds those fits and the folds and is one more
``LogProbJudge``: every member runs its own forward passes on its own held-out rows (``NeuralNetClassifier._forward_logp``: under
its gate, on its stream), one ``ops.scatter_logp`` launch per member writes them -- at that member's temperature -- into one
float32 [N, V] buffer, and ``reliability``, ``ranking``, ``error_analysis``, ``score_interval``, ``compare``, ``risk_coverage`` and the
rest, ``label_issues`` above all, then judge all N rows through the same ``_forward_logp(ds, then)`` hook.  Nothing is assembled on
the host and no torch arithmetic runs on the device.

What is out of fold is the log-probs of the cross-fitted rows and of those alone: the methods that take new rows (``predict``,
``predict_set``, ``predict_selective`` on other data) are not defined here -- ``ensemble()`` gives the ``VotingEnsemble`` of the
members for that.  Not here either: ``ShardedGridSearchCV`` keeping its fold fits (it runs exactly these fits and keeps no
predictions) and lockstep cross-fitting; ``cross_fit`` fits the folds one after the other.

As for ``PriorShift``: the reference Transformer feeds the gold label to its decoder (reproduced
for parity), so its log-probs of a row depend on that row's label even out of fold.  For it a label audit is a statement about the
log-probs, not about the labels; it is meaningful for the two RNN models."""
import numpy as np
import torch
from sklearn.base import BaseEstimator, ClassifierMixin

from . import ops
from .data import TokenDataset
from .ensemble import VotingEnsemble
from .judge import LogProbJudge
from .net import stream_sync


def check_partition(what, folds):
    """``folds`` as a list of int64 index arrays that together hold every index of ``range(N)`` exactly once; anything else raises
    ValueError.  Returns ``(folds, N)``."""
    try:
        folds = [np.ascontiguousarray(np.asarray(f), dtype=np.int64) for f in folds]
    except (TypeError, ValueError):
        folds = None
    if not folds or not all(f.ndim == 1 and f.size > 0 for f in folds):
        raise ValueError(f"{what}: folds must be a list of non-empty 1-D index arrays, one per member")
    every = np.concatenate(folds)
    N = int(every.size)
    if not np.array_equal(np.sort(every), np.arange(N)):
        raise ValueError(f"{what}: the folds must partition range({N}): every row in exactly one fold ({N} indices, "
                         f"{np.unique(every).size} distinct, from {int(every.min())} to {int(every.max())})")
    return folds, N


class OutOfFold(LogProbJudge, ClassifierMixin, BaseEstimator):
    """``members``: initialised ``NeuralNetClassifier``s on one device with equal ``classes_`` (``VotingEnsemble``'s checks);
    ``folds``: per member the indices of the rows it did NOT see -- together a partition of ``range(N)``, otherwise ValueError.
    ``dataset``: the ``TokenDataset`` the indices refer to; ``_forward_logp`` then refuses every other one (length, labels,
    lengths and ids are compared) -- without it only the length can be.  ``calibrated``: a member that fitted a temperature enters
    as softmax(z / T_k), one with a ``bias_temperature`` calibration as softmax(beta_k z + b_k); False: every member at
    T = 1.  It has no temperature of its own: ``calibration_`` is None,
    ``temperature_`` 1.0."""
    calibration_ = None
    temperature_ = 1.0
    predict_nonlinearity = "auto"
    initialized_ = True

    def __init__(self, members, folds, dataset=None, calibrated=True):
        checked = VotingEnsemble(members)                    # the members' checks, written once
        folds, N = check_partition("OutOfFold", folds)
        if len(folds) != len(checked.members):
            raise ValueError(f"OutOfFold: {len(checked.members)} members and {len(folds)} folds: one held-out fold per member")
        if dataset is not None and not (isinstance(dataset, TokenDataset) and len(dataset) == N):
            raise ValueError(f"OutOfFold: dataset must be the TokenDataset of the {N} rows the folds partition")
        self.members, self.folds, self.dataset, self.calibrated = checked.members, folds, dataset, bool(calibrated)
        self.classes_ = checked.classes_
        self.rows_ = N

    def ensemble(self, **kw):
        """``VotingEnsemble(members, **kw)``: what to predict NEW rows with."""
        return VotingEnsemble(self.members, **kw)

    def attribute(self, *args, **kwargs):
        raise NotImplementedError("OutOfFold.attribute: out-of-fold log-probs exist only for the cross-fitted rows themselves, not for "
                                  "occluded variants of them; attribute with a member or with ensemble()")

    def _refuse_other_data(self, ds):
        own = self.dataset
        same = len(ds) == self.rows_ and (own is None or ds is own or (np.array_equal(ds.y, own.y) and np.array_equal(ds.lengths, own.lengths)
                                                                       and np.array_equal(ds.ids, own.ids)))
        if not same:
            raise ValueError(f"OutOfFold: out-of-fold log-probs exist only for the {self.rows_} rows that were cross-fitted on, in their "
                             f"order; got a dataset of {len(ds)} rows" + ("" if len(ds) != self.rows_ else " with other contents")
                             + " (ensemble() predicts new rows)")

    def _forward_logp(self, ds, then):
        """The out-of-fold float32 log-probs [N, V] of the cross-fitted rows on the device, handed to ``then(logp, y_dev)``: the
        hook every consumer of ``LogProbJudge`` goes through.  Each member's own ``_forward_logp`` on its held-out rows first --
        under its gate, on its stream, returned once that stream has drained -- then, on the first member's stream and under
        its gate, one ``ops.scatter_logp`` per member into one buffer."""
        self._refuse_other_data(ds)

        def keep(member):                                    # (a bias calibration is already in the log-probs: VotingEnsemble's rule)
            def then(logp, yd):
                logp = logp if logp.dtype == torch.float32 else logp.float()
                return member._calibrated_logp(logp, member._uses_temperature(self.calibrated))
            return then
        got = [m._forward_logp(ds[idx], keep(m)) for m, idx in zip(self.members, self.folds)]
        first = self.members[0]
        first._gate.enter(not first._fused)
        try:
            first._enter_stream()
            with torch.cuda.stream(first._stream), torch.no_grad():
                dev = got[0][0].device
                out = torch.empty(self.rows_, got[0][0].shape[1], dtype=torch.float32, device=dev)     # every row is written: a partition
                for (logp, state), idx in zip(got, self.folds):
                    ops.scatter_logp(logp, torch.from_numpy(idx).to(dev), out, state=state)
                res = then(out, torch.from_numpy(np.asarray(ds.y)).to(dev))
            stream_sync(first._stream)
        finally:
            first._gate.leave(not first._fused)
        return res


def cross_fit_folds(dataset, cv):
    """``cross_fit``'s folds ``[(train, held_out), ...]``: ``StratifiedKFold(cv)`` without shuffle on the labels -- with ``groups`` on
    the dataset ``data.group_folds`` (``StratifiedGroupKFold(cv)`` without shuffle), as ``grid.build_tasks`` cuts them"""
    y = np.asarray(dataset.y)
    if getattr(dataset, "groups", None) is not None:
        from .data import group_folds
        return group_folds("cross_fit", "cv", y, dataset.groups, cv)
    from sklearn.model_selection import StratifiedKFold
    return list(StratifiedKFold(n_splits=cv).split(np.zeros(len(y)), y))


def cross_fit(estimator, dataset, cv=5, seed=None, calibrated=True):
    """Cross-fit ``estimator`` on ``dataset`` and return the ``OutOfFold``: ``StratifiedKFold(cv)`` without shuffle on the dataset's
    labels -- ``grid.build_tasks``' splitter, so the folds are the grid search's -- and per fold a ``sklearn.base.clone`` of the
    estimator fitted on the other folds, one after the other.  ``seed``: ``torch.manual_seed(seed + f)`` before fold f's clone
    initialises (None: torch's generator as it stands).  ``calibrated``: as in ``OutOfFold``.  A dataset that carries ``groups``
    (``with_groups``) is cut by ``cross_fit_folds`` instead: no group of near-duplicates straddles a fold, and each clone's internal
    valid split keeps them whole too (the slices carry the groups)."""
    from sklearn.base import clone
    if not isinstance(dataset, TokenDataset):
        raise TypeError("cross_fit: dataset must be a slnlp.data.TokenDataset")
    cv = ops._int_in("cross_fit", "cv", cv, 2, ops._lib.ENSEMBLE_MAX_MEMBERS)
    if seed is not None:
        seed = ops._int_in("cross_fit", "seed", seed, 0, 2 ** 63 - 1 - cv)
    members, folds = [], []
    for f, (train, held_out) in enumerate(cross_fit_folds(dataset, cv)):
        if seed is not None:
            torch.manual_seed(seed + f)
        members.append(clone(estimator).fit(dataset[train]))
        folds.append(held_out)
    return OutOfFold(members, folds, dataset=dataset, calibrated=calibrated)
