"""skorch-shaped estimator around the HIP modules.

The reference trains through ``skorch.NeuralNetClassifier(**net_params)``
(/root/reference/main.py:44, helper.py:41-105) driven by sklearn.  skorch is
not available here, and its Python step loop is exactly the per-batch overhead
the hot path removes, so this class restates the pieces of skorch 0.10 the
reference configures, with the same parameter names
(``module__*``, ``optimizer__*``, ``criterion__*``, ``lr``, ``max_epochs``,
``batch_size``, ``device``, ``callbacks``-level settings) and the same fit-loop
semantics:

* internal 80/20 stratified split, first fold of ``StratifiedKFold(5)`` (skorch ``CVSplit(5)``);
* batches in dataset order (``shuffle`` is commented out, helper.py:75-76), or -- ``iterator_train__shuffle=True`` -- in the
  order torch's ``RandomSampler`` draws per epoch (slnlp/sampler.py); ``iterator_train__drop_last`` drops the short last batch;
  ``iterator_train__balance=True`` makes every train epoch a class-balanced resample of the fit's own train split, drawn on
  the device (csrc/balance.hip) -- the valid split is never touched, and ``iterator_train__shuffle`` has nothing left to do;
  ``iterator_train__augment={"frame_drop": p, "token_mask": p}`` shows every train epoch a freshly augmented copy of the train
  rows, drawn on the device (csrc/augment.hip): random timesteps deleted, random tokens replaced by ``<unk>`` -- valid, test and
  predict data are never augmented, and the train scores are the training pass's (augmented inputs), as under dropout;
* per batch: forward -> CrossEntropyLoss(ignore_index=pad) -> backward ->
  clip_grad_norm_(gradient_clip_value) -> SGD(momentum)  == ONE hipGraph replay;
* per epoch: valid pass, ``EpochScoring`` metrics for train/valid, ``lr`` scoring,
  ``LRScheduler`` (``ReduceLROnPlateau`` on valid_loss, or any other ``torch.optim.lr_scheduler`` policy stepped per
  epoch or per batch: slnlp/schedule.py), ``EarlyStopping`` (patience,
  relative threshold), ``Checkpoint`` on ``valid_loss_best`` (helper.py:197-273);
* ``weight_averaging={...}``: a running average of the weights (SWA / EMA, ``torch.optim.swa_utils``) kept on the device beside
  the model, fed per epoch or per batch, and -- ``predict`` -- what ``predict_proba`` / ``predict`` / ``score`` evaluate with;
* ``calibration={"method": "temperature"}``: at the end of a fit one temperature is fitted on the valid split's log-probs, on
  the device (csrc/calibration.hip), and ``predict_proba`` returns ``softmax(z / T)``; ``predict`` and the history never change;
  ``{"method": "bias_temperature", "bias_sd": 2.0}`` fits a shrunk per-class bias beside it (csrc/bias_calibration.hip) and
  ``predict_proba`` returns ``softmax(beta z + b)``: the history never changes, ``predict`` is the calibrated arg-max and can;
* ``conformal={"alpha": 0.1, ...}``: at the end of a fit, after the temperature, the threshold of split conformal prediction sets
  (LAC / APS / RAPS, csrc/conformal.hip) is taken on the valid split's log-probs, on the device; ``predict_set`` then returns per
  sample the set of classes that holds the true one with probability about 1 - alpha.  About: the valid split also chose the
  temperature and the stopping epoch, so the guarantee is approximate there; it is exact only with ``conformalize`` on rows the
  fit never saw (``coverage`` reports what the sets achieve on labelled data);
* ``train_dynamics=True``: every epoch's train log-probs are folded, on the device, into per-row integer counts
  (csrc/train_dynamics.hip: two queued launches per epoch, no host wait), and ``train_dynamics()`` reports which train rows the
  fit never learned, learned and forgot, wavers on, or fits only against a large negative margin (confidence / variability /
  correctness, forgetting events, AUM).  The probabilities are the training pass's: dropout on, augmented inputs under
  ``iterator_train__augment``, each visit under the weights of its own step.  Off (the default), nothing is allocated or queued.

Beyond skorch: ``reliability`` (ECE / MCE / Brier, csrc/reliability.hip), ``predict_topk`` and ``error_analysis`` (top-k classes,
confusion matrix, most-confused pairs, per-class report: csrc/confusion.hip) and ``ranking`` (one-vs-rest ROC AUC and average
precision per class, csrc/ranking.hip) reduce a fitted estimator's log-probs on the device; ``conformalize`` / ``predict_set`` /
``coverage`` (csrc/conformal.hip) say something about a single sample; ``risk_coverage`` / ``fit_rejection`` /
``predict_selective`` (csrc/selective.hip) let the fit decline to answer below a confidence threshold.

The compute path is HIP only; with no GPU ``fit`` / ``predict`` raise.
"""
import threading
import json
import warnings
import os
import time
import importlib

import numpy as np
import torch

from . import metrics, ops, param_groups, sampler, schedule
from .data import DeviceRows
from .judge import CONFORMAL_DEFAULTS, LogProbJudge, conformal_least_rows, conformal_options  # noqa: F401  (part of this module's names)


# module construction consumes torch's global CPU generator (initial weights): concurrent fits take turns
INIT_LOCK = threading.RLock()

# Which stream a fit runs on.  "thread" (default): one stream per host thread and device for FUSED fits -- fits whose every
# kernel is this library's (fused SGD / Adam step, slnlp.lockstep): the grid search's `fits_per_gpu` host threads feed separate
# hardware queues, so one unit's small launches (the decoder's [B, E] chain, the optimizer) run beside another's; measured +17 %
# folds/hr on bench.py's grid sample, scores bit-identical (bench.py prints their CRC-32).  "device": one stream per device for
# every estimator of the process (round 2's rule, SLNLP_STREAM_MODE=device).
# History: round 2 measured that fits on several queues changed each other's results and shipped the
# one-stream rule.  Round 3 found the cause -- packed fp32 VALU instructions compute wrongly when a workgroup of another kernel
# shares the CU -- and builds the library without them.  torch's own kernels (and rocBLAS) ARE built with packed fp32, so
# whatever runs them never shares the GPU with another fit here:
#   * a fit that steps through torch (another optimizer / criterion: `_fused` False) runs on the shared device stream and holds
#     the device EXCLUSIVELY for its fit / predict calls (`_DeviceGate`: fused fits of other threads hold it shared);
#   * the scoring softmax of `predict_proba` runs on the host copy of the log-probs (torch's CPU op, what the reference runs);
#   * what is left on the GPU from torch beside other fits moves or compares bits (copies, cat, argmax, gather): no fp32 arithmetic.
# The library-wide stream policy is never flipped from here: a thread that gets a stream of its own opts ITS steps out
# (slnlp_set_thread_stream_policy).
STREAM_MODE = os.environ.get("SLNLP_STREAM_MODE", "thread")      # "thread" | "device"
_DEVICE_STREAMS = {}
_DEVICE_STREAMS_LOCK = threading.Lock()


class _DeviceGate:
    """Readers-writer gate per device: fused fits enter shared, fits that run torch kernels enter exclusive (writer
    preference, re-entrant per thread for nested fit -> predict calls)."""
    def __init__(self):
        self._cv = threading.Condition()
        self._shared, self._excl_owner, self._excl_depth, self._excl_waiting = 0, None, 0, 0
        self._tl = threading.local()

    def enter(self, exclusive):
        me = threading.get_ident()
        with self._cv:
            if self._excl_owner == me:                       # nested call of the exclusive holder
                self._excl_depth += 1
                return
            depth = getattr(self._tl, "shared", 0)
            if not exclusive and depth:                      # nested shared call
                self._tl.shared = depth + 1
                return
            if exclusive and depth:
                # this thread already holds the gate SHARED (it is inside a fused fit): waiting for "no shared holders" would wait for
                # itself, for ever.  A torch-stepped fit / predict nested in a fused fit of the same thread has no legal order.
                raise RuntimeError("slnlp device gate: a fit or predict that steps through torch kernels (exclusive use of the GPU) was "
                                   "started from inside a fused fit of the same thread (shared use): finish the fused fit first, or run "
                                   "the other estimator from a thread of its own")
            if exclusive:
                self._excl_waiting += 1
                while self._excl_owner is not None or self._shared:
                    self._cv.wait()
                self._excl_waiting -= 1
                self._excl_owner, self._excl_depth = me, 1
            else:
                while self._excl_owner is not None or self._excl_waiting:
                    self._cv.wait()
                self._shared += 1
                self._tl.shared = 1

    def leave(self, exclusive):
        with self._cv:
            if self._excl_owner == threading.get_ident():
                self._excl_depth -= 1
                if self._excl_depth == 0:
                    self._excl_owner = None
                    self._cv.notify_all()
                return
            self._tl.shared -= 1
            if self._tl.shared == 0:
                self._shared -= 1
                self._cv.notify_all()


_GATES = {}


def device_gate(dev):
    dev = torch.device(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with _DEVICE_STREAMS_LOCK:
        g = _GATES.get(idx)
        if g is None:
            g = _GATES[idx] = _DeviceGate()
        return g


def stream_sync(stream):
    """Wait for what THIS thread has queued on the shared stream so far -- not for the whole device: with several host
    threads feeding one stream, torch.cuda.synchronize() would also wait for everything the others queue in the meantime."""
    ev = torch.cuda.Event()
    ev.record(stream)
    ev.synchronize()


def device_stream(dev, per_thread=None):
    """The stream a fit on `dev` runs on: this host thread's own (`per_thread`, default: STREAM_MODE == "thread") or the one
    every estimator of the process shares on that device.  A thread that gets a stream of its own also opts its library steps
    out of the one-sequence-per-device ordering (thread-scoped: slnlp_set_thread_stream_policy)."""
    dev = torch.device(dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if per_thread is None:
        per_thread = STREAM_MODE == "thread"
    key = (dev.index, threading.get_ident()) if per_thread else dev.index
    with _DEVICE_STREAMS_LOCK:
        st = _DEVICE_STREAMS.get(key)
        if st is None:
            st = _DEVICE_STREAMS[key] = torch.cuda.Stream(device=dev)
    if per_thread:
        from . import _lib
        _lib.load().slnlp_set_thread_stream_policy(0)
    return st


def release_thread_streams():
    """Drop the calling thread's per-thread streams (a grid worker thread about to exit) and put its library steps back under
    the process-wide stream policy."""
    me = threading.get_ident()
    with _DEVICE_STREAMS_LOCK:
        for key in [k for k in _DEVICE_STREAMS if isinstance(k, tuple) and k[1] == me]:
            del _DEVICE_STREAMS[key]
    from . import _lib
    _lib.load().slnlp_set_thread_stream_policy(-1)


_RESOLVED = {}


def _resolve(obj):
    """Dotted name -> object ("model.Transformer", "torch.optim.SGD"; helper.py resolves its config strings with
    pydoc.locate).  Not pydoc.locate itself: its safeimport() parks sys.exc_info() in a local, and that traceback <-> frame
    cycle keeps every CALLER frame -- the estimator being initialised, the whole list of a lockstep unit's estimators and
    their GPU arenas -- alive until the cyclic GC happens to run (measured: 1.5 GB per grid work unit, 170 GB peak)."""
    if not isinstance(obj, str):
        return obj
    if obj in _RESOLVED:
        return _RESOLVED[obj]
    parts = obj.split(".")
    found = None
    for i in range(len(parts) - 1, 0, -1):               # longest importable module prefix, then attributes
        try:
            found = importlib.import_module(".".join(parts[:i]))
        except ImportError:
            continue
        for name in parts[i:]:
            found = getattr(found, name, None)
            if found is None:
                break
        if found is not None:
            break
    if found is None and len(parts) == 1:
        try:
            found = importlib.import_module(obj)
        except ImportError:
            found = None
    if found is not None:
        _RESOLVED[obj] = found
    return found


def fused_kind(criterion, opt_cls, opt_kwargs, module_cls, groups=None):
    """Which fused clip + update kernel replaces the torch optimizer of a fit: "sgd", "adam", "adamw", or None (the fit steps
    through torch).  ``criterion`` is the constructed criterion; a ``CrossEntropyLoss`` argument the fused criterion does not
    implement (``reduction="none"``) sends the fit to the torch path -- it is never dropped.  The optimizer arguments are
    checked by constructing the torch optimizer on a dummy parameter, so bad ones raise torch's own error here.
    ``groups``: the ``optimizer__param_groups`` pairs (``optimizer_kwargs`` splits them off): every pair's settings are
    checked the same way; the fit stays fused while they only name ``lr`` / ``weight_decay`` -- any other per-group key
    (``momentum``, ``betas``, ...) sends it to the torch path, like ``reduction="none"``."""
    groups = param_groups.as_pairs(groups)
    for _, settings in groups:
        optimizer_defaults(opt_cls, {**opt_kwargs, **settings})
    if not isinstance(criterion, torch.nn.CrossEntropyLoss) or not hasattr(module_cls, "engine"):
        return None
    if criterion_options(criterion) is None:
        return None
    kinds = {torch.optim.SGD: "sgd", torch.optim.Adam: "adam", torch.optim.AdamW: "adamw"}
    kind = kinds.get(opt_cls)
    if kind is None:
        return None
    d = optimizer_defaults(opt_cls, opt_kwargs)
    if d.get("maximize", False) or (kind != "sgd" and d.get("amsgrad", False)):
        return None
    if not param_groups.fused_ok(groups):
        return None
    return kind


def criterion_options(criterion):
    """The fused criterion's settings of a ``CrossEntropyLoss`` ({weight, label_smoothing, reduction}, the keywords of the
    engines' ``set_criterion``), or None when it asks for something the fused criterion does not implement.  ``ignore_index``
    is the vocabulary's pad index on the fused path, as the reference always passes it."""
    if not isinstance(criterion, torch.nn.CrossEntropyLoss) or criterion.reduction not in ("mean", "sum"):
        return None
    w = criterion.weight
    if w is not None and (w.dim() != 1 or not w.is_floating_point()):
        return None
    return {"weight": None if w is None else w.detach().float().cpu(), "label_smoothing": float(criterion.label_smoothing),
            "reduction": criterion.reduction}


def optimizer_kwargs(opt_kwargs):
    """(constructor keywords, ``param_groups`` pairs) of the ``optimizer__*`` settings: ``param_groups`` is skorch's, not a
    keyword of any torch optimizer."""
    kw = dict(opt_kwargs)
    return kw, param_groups.as_pairs(kw.pop("param_groups", None))


def optimizer_defaults(opt_cls, opt_kwargs):
    """The optimizer's settings with torch's defaults filled in (AdamW's weight_decay is 1e-2, Adam's 0): construct it on a
    dummy parameter -- which also raises torch's own error for an invalid combination (nesterov with dampening)."""
    kw = dict(opt_kwargs)
    kw.setdefault("lr", 0.01)
    return dict(opt_cls([torch.nn.Parameter(torch.zeros(1))], **kw).defaults)


def update_options(kind, defaults):
    """The engines' ``set_update`` keywords for a fused fit."""
    if kind == "sgd":
        return {"kind": "sgd", "dampening": float(defaults.get("dampening", 0.0)), "weight_decay": float(defaults.get("weight_decay", 0.0)),
                "nesterov": bool(defaults.get("nesterov", False))}
    return {"kind": kind, "weight_decay": float(defaults.get("weight_decay", 0.0))}     # the fit's own in a lockstep group


AVERAGING_KEYS = ("kind", "decay", "every", "start_epoch", "predict")


def averaging_options(setting):
    """The ``weight_averaging`` setting with its defaults filled in -- {kind "swa" | "ema", decay (ema only; 0.999), every
    "epoch" | "batch", start_epoch >= 1, predict} -- or None (off).  Anything the fit loop could not honour raises ValueError here."""
    if setting is None or setting is False:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"weight_averaging={setting!r}: expected a dict with keys among {AVERAGING_KEYS} or None")
    unknown = sorted(set(setting) - set(AVERAGING_KEYS))
    if unknown:
        raise ValueError(f"weight_averaging: unknown keys {unknown} (known: {AVERAGING_KEYS})")
    kind = setting.get("kind", "swa")
    if kind not in ("swa", "ema"):
        raise ValueError(f"weight_averaging: kind={kind!r}, expected 'swa' or 'ema'")
    decay = setting.get("decay", 0.999 if kind == "ema" else 0.0)
    if kind == "ema" or "decay" in setting:
        if isinstance(decay, bool) or not isinstance(decay, (int, float, np.floating)) or not 0.0 < float(decay) < 1.0:
            raise ValueError(f"weight_averaging: decay={decay!r} outside (0, 1)")
    every = setting.get("every", "epoch")
    if every not in ("epoch", "batch"):
        raise ValueError(f"weight_averaging: every={every!r}, expected 'epoch' or 'batch'")
    start = setting.get("start_epoch", 1)
    if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or int(start) < 1:
        raise ValueError(f"weight_averaging: start_epoch={start!r}, expected an integer >= 1")
    predict = setting.get("predict", True)
    if not isinstance(predict, (bool, np.bool_)):
        raise ValueError(f"weight_averaging: predict={predict!r}, expected True or False")
    return {"kind": kind, "decay": float(decay) if kind == "ema" else 0.0, "every": every, "start_epoch": int(start),
            "predict": bool(predict)}


CALIBRATION_KEYS = ("method",)
BIAS_CALIBRATION_KEYS = ("method", "bias_sd")
BIAS_SD_DEFAULT = 2.0


def calibration_options(setting):
    """The ``calibration`` setting with its defaults filled in -- {method "temperature"} -- or None (off).  Anything else raises
    ValueError here.

    ``{"method": "bias_temperature", "bias_sd": 2.0}`` fits a per-class bias beside the temperature, softmax(beta z + b)
    (``ops.fit_bias_temperature``: bias-corrected temperature scaling, which removes the per-class offset of a fit trained under
    other class priors than it is judged under).  ``bias_sd``, a key of this method only, is the standard deviation of the
    Gaussian prior on every bias: a finite number > 0, small values shrink the bias towards a temperature alone.  Its default 2.0
    is a design choice, not a measurement -- e^2 is a prior ratio of about 7 to 1 within one standard deviation -- and the value
    is a grid axis a search can rank on ``neg_log_loss``."""
    if setting is None or setting is False:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"calibration={setting!r}: expected a dict with keys among {CALIBRATION_KEYS} or None")
    method = setting.get("method", "temperature")
    if method == "bias_temperature":
        unknown = sorted(set(setting) - set(BIAS_CALIBRATION_KEYS))
        if unknown:
            raise ValueError(f"calibration: unknown keys {unknown} (known for method 'bias_temperature': {BIAS_CALIBRATION_KEYS})")
        sd = setting.get("bias_sd", BIAS_SD_DEFAULT)
        if isinstance(sd, (bool, np.bool_)) or not isinstance(sd, (int, float, np.integer, np.floating)) or not 0.0 < float(sd) < float("inf"):
            raise ValueError(f"calibration: bias_sd={sd!r}, expected a finite number > 0")
        return {"method": "bias_temperature", "bias_sd": float(sd)}
    unknown = sorted(set(setting) - set(CALIBRATION_KEYS))
    if unknown:
        raise ValueError(f"calibration: unknown keys {unknown} (known: {CALIBRATION_KEYS})")
    if method != "temperature":
        raise ValueError(f"calibration: method={method!r}, expected 'temperature'")
    return {"method": "temperature"}


def calibration_to_json(info):
    """``calibration_`` as ``calibration.json`` holds it: the bias of a ``bias_temperature`` fit as a list (repr round-trips a
    double bit for bit); a temperature fit's dict as it is."""
    return {k: (np.asarray(v, dtype=np.float64).tolist() if k == "bias" else v) for k, v in info.items()}


def calibration_from_json(info):
    """``calibration_to_json``'s inverse: the bias back as float64 [V]."""
    return {k: (np.asarray(v, dtype=np.float64) if k == "bias" else v) for k, v in info.items()}


def fit_calibration(opts, logp, y):
    """Queue the fit of the ``calibration`` option ``opts`` on the device log-probs ``logp`` and labels ``y`` (current stream, no
    host wait): what ``download_calibration`` takes."""
    if opts["method"] == "bias_temperature":
        return ops.fit_bias_temperature(logp, y, bias_sd=opts["bias_sd"])
    return ops.fit_temperature(logp, y)


def download_calibration(opts, fitted):
    """``(info, state, bias)`` of ``fit_calibration``'s result: the host dict (it waits for the fit's launches), the device state
    and the device bias (None for a temperature)."""
    if opts["method"] == "bias_temperature":
        state, bias = fitted
        return ops.bias_temperature_download(state, bias, opts["bias_sd"]), state, bias
    return ops.temperature_download(fitted), fitted, None


def next_n_averaged(opts, history, n_batches):
    """``n_averaged`` of the epoch about to join ``history``: the models in the average once that epoch is over, from the cadence
    and the rows alone (no device read) -- the last row's count plus, from ``start_epoch`` on, one per epoch or one per train
    batch.  A resumed fit goes on from the count its loaded history ends with."""
    have = int(history[-1].get("n_averaged", 0)) if history else 0
    if len(history) + 1 < opts["start_epoch"]:
        return have
    return have + (1 if opts["every"] == "epoch" else int(n_batches))


def adam_args(net):
    """(betas, eps, weight_decay) of a fused Adam / AdamW fit, torch's defaults filled in."""
    d = net._opt_defaults
    return tuple(float(b) for b in d["betas"]), float(d["eps"]), float(d["weight_decay"])


class ScoringWrapper:
    """Named sklearn scorer with the extra keyword the reference gives each metric (helper.py:529-554): log-loss is told
    the full label set (a fold may miss classes), the precision / recall / F1 family gets ``zero_division=0``, accuracy
    takes nothing.  Beyond the reference's names: ``balanced_accuracy`` takes nothing either, and the top-k family --
    ``top_k_accuracy`` (sklearn's k = 2) and ``top<k>_accuracy`` for any k >= 1, a ``top_k_accuracy_score`` scorer with that
    k -- is told the label set like log-loss.  The calibration family (``metrics.CALIBRATION``: ``neg_ece``, ``neg_ece<B>``,
    ``neg_mce``, ``neg_brier``), which sklearn does not have, is a ``make_scorer`` of ``metrics.calibration_error`` on
    ``predict_proba`` with ``greater_is_better=False`` -- sign -1, like ``neg_log_loss`` -- and is told the label set too.
    The ranking family (``metrics.RANKING``: ``auc_macro``, ``auc_weighted``, ``ap_macro``, ``ap_weighted``) is a ``make_scorer``
    of ``metrics.ranking_score`` on ``predict_proba``, greater is better, told the label set as well.
    Exposes ``score`` (the name) and ``greater_is_better`` -- what the reference's EpochScoring and GridSearchCV wiring read
    (helper.py:255-268, 183-194)."""

    _EXTRA = {"neg_log_loss": lambda labels: {"labels": labels}, "accuracy": lambda labels: {},
              "balanced_accuracy": lambda labels: {}, "top_k_accuracy": lambda labels: {"labels": labels}}

    def __init__(self, score_func, labels=None):
        from sklearn.metrics import get_scorer, make_scorer, top_k_accuracy_score
        self.score = score_func
        k = metrics.top_k_of(score_func)
        cal = metrics.calibration_metric_of(score_func)
        if cal is not None:
            base = make_scorer(metrics.calibration_error, greater_is_better=False, response_method="predict_proba", kind=cal[0], bins=cal[1])
            extra = {"labels": labels}
        elif score_func in metrics.RANKING:
            base = make_scorer(metrics.ranking_score, greater_is_better=True, response_method="predict_proba", name=score_func)
            extra = {"labels": labels}
        elif k is not None and score_func != "top_k_accuracy":
            # what sklearn's own "top_k_accuracy" scorer is, with the name's k
            base = make_scorer(top_k_accuracy_score, greater_is_better=True, response_method=("decision_function", "predict_proba"), k=k)
            extra = {"labels": labels}
        else:
            base = get_scorer(score_func)
            extra = self._EXTRA.get(score_func, lambda labels: {"zero_division": 0})(labels)
        self.greater_is_better = base._sign > 0
        # a scorer object of the same kind with the merged keywords (get_scorer hands out a fresh copy per call)
        base._kwargs = {**base._kwargs, **extra}
        self.scorer = base

    @staticmethod
    def needs_labels(score_func):
        """Whether the scorer must be told the full label set: a test fold may miss classes the probability columns stand for."""
        return (score_func == "neg_log_loss" or metrics.top_k_of(score_func) is not None
                or metrics.calibration_metric_of(score_func) is not None or score_func in metrics.RANKING)

    def __call__(self, estimator, X, y_true, sample_weight=None):
        return self.scorer(estimator, X, y_true, sample_weight)

    def __repr__(self):
        return "%s('%s')" % (type(self).__name__, self.score)


from sklearn.base import BaseEstimator, ClassifierMixin  # noqa: E402  (sklearn >= 1.6 scorers require classifier tags)


class _CachedPredictor(ClassifierMixin, BaseEstimator):
    """What skorch's score caching gives EpochScoring: predictions already made during the epoch."""

    def __init__(self, proba, classes):
        self._proba, self.classes_ = proba, classes

    def predict_proba(self, X):
        return self._proba

    def predict(self, X):
        return self.classes_[self._proba.argmax(-1)]


class _FitRun:
    """One estimator's fit between epochs: the internal split, the device-resident data, and skorch's per-epoch callbacks
    (EpochScoring on the cached predictions, Checkpoint, LRScheduler, EarlyStopping; helper.py:197-273).
    ``partial_fit`` drives one of these with its own batch loop; ``slnlp.lockstep`` drives K of them with one launch
    sequence per step -- the epoch bookkeeping is this one piece of code either way."""

    def __init__(self, net, ds):
        self.net = net
        net.classes_ = np.arange(len(ds.vocab_y)) if ds.vocab_y is not None else np.arange(int(ds.y.max()) + 1)
        labels = net.labels if net.labels is not None else ds.labels()
        idx_tr, idx_va = net._train_split(ds)
        self.tr, self.va = ds[idx_tr], (ds[idx_va] if idx_va is not None else None)
        self.idx_tr = idx_tr
        self.Xtr, self.Ltr, self.ytr = net._device_data(self.tr)
        if self.va is not None:
            self.Xva, self.Lva, self.yva = net._device_data(self.va)
        self.wrappers = [ScoringWrapper(s, labels) for s in (net.scoring or [])]
        # the fast metrics index the probability columns by class id: valid when the labels are exactly the columns
        self.fast_ok = labels is not None and list(labels) == list(range(len(net.classes_)))
        self._score_out = {}                                 # split -> the reduction's device buffers (ops.score_rows)
        self._rel_out = {}                                   # split -> {bins: ops.reliability_rows' device buffers}
        self._rank_out = {}                                  # split -> ops.ranking_rows' device buffers (the table alone)
        es, clip, sched = net.early_stopping, net.gradient_clipping, net.lr_scheduler
        self.es = es
        self.max_norm = float(clip["gradient_clip_value"]) if clip and clip.get("gradient_clip_value") else 0.0
        self.momentum = float(net._opt_kwargs.get("momentum", 0.0))
        self.plateau, self.schedule, self.epoch_lrs = None, None, None
        if sched and not schedule.is_plateau(sched):
            # the schedule's position is a function of the history: built from scratch and replayed up to where the fit stands
            self.schedule = schedule.LRSchedule.from_setting(sched, net._base_lrs()).fast_forward(net.history)
            net._set_lr(self.schedule.rates)
        elif sched:
            # one dummy group per param group, at the groups' current rates (min_lr / factor lists apply per group, as in torch)
            dummy = torch.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": v} for v in net.lrs_], lr=net.lr_)
            self.plateau = torch.optim.lr_scheduler.ReduceLROnPlateau(
                dummy, **{k: v for k, v in sched.items() if k not in ("policy", "monitor", "step_every")})
        self.best_valid, self.misses, self.dyn_thr = float("inf"), 0, float("inf")
        self.bs = int(net.batch_size)
        # the train iterator: which rows an epoch visits (all, or the full batches) and in which order (dataset order, or a
        # fresh draw of torch's RandomSampler per epoch); valid and test passes stay in dataset order
        self.shuffle, self.drop_last = net._iterator_train()
        self.n_visit = sampler.n_visit(len(self.tr), self.bs, self.drop_last)
        if self.n_visit < 1:
            raise ValueError(f"iterator_train__drop_last=True with {len(self.tr)} train rows and batch_size {self.bs}: no full batch, "
                             "nothing to train on")
        self.sampler = None
        # iterator_train__balance: a class-balanced resample of the train rows per epoch, drawn on the device into the order
        # table (slnlp_balanced_order).  The plan holds the class tables of THIS fit's train labels; the epoch length -- the same
        # every epoch -- is the plan's.  The draw permutes, so the shuffling sampler is not built beside it.
        self.balance = None
        if net._iterator_train_balance():
            self.balance = ops.BalancePlan(self.tr.y, max(len(net.classes_), int(self.tr.y.max()) + 1))
            self.n_visit = sampler.n_visit(self.balance.rows, self.bs, self.drop_last)
            if self.n_visit < 1:
                raise ValueError(f"iterator_train__drop_last=True with {self.balance.rows} balanced train rows and batch_size {self.bs}: "
                                 "no full batch, nothing to train on")
            # the draw is a function of (seed, epoch number): the seed rides the epoch rows, a resumed fit needs nothing else
            seed = sampler.seed_of(net.history, "balance_seed")
            if seed is None:                                 # (balancing switched on after initialize(): drawn now)
                seed = net.balance_seed_ if getattr(net, "balance_seed_", None) is not None else sampler.draw_seed()
            net.balance_seed_ = seed
            dev = self.ytr.device
            self._bal_out = (torch.empty(self.balance.rows, dtype=torch.int64, device=dev),
                             torch.empty(self.balance.rows, dtype=torch.int64, device=dev))
        elif self.shuffle:
            # the order's position is a function of the history, like a schedule's: the seed rides the epoch rows
            seed = sampler.seed_from_history(net.history)
            if seed is None:                                 # (shuffling switched on after initialize(): drawn now)
                seed = net.shuffle_seed_ if getattr(net, "shuffle_seed_", None) is not None else sampler.draw_seed()
            net.shuffle_seed_ = seed
            self.sampler = sampler.EpochOrder(len(self.tr), self.bs, net.shuffle_seed_, self.drop_last).fast_forward(len(net.history))
        self.epoch_order, self.order_dev, self.y_visit_dev = None, None, None
        # iterator_train__augment: the pristine device copy of the train split stays here; Xtr / Ltr become two buffers of the same
        # shapes, allocated once, that order() refills every epoch (slnlp_augment_rows) -- dataset-order slices, gather launches,
        # captured graphs and a lockstep group's data pointers all keep reading the same addresses
        self.augment = net._iterator_train_augment()
        if self.augment is not None:
            seed = sampler.seed_of(net.history, "augment_seed")
            if seed is None:                                 # (the option switched on after initialize(): drawn now)
                seed = net.augment_seed_ if getattr(net, "augment_seed_", None) is not None else sampler.draw_seed()
            net.augment_seed_ = seed
            self._aug_ids = net._augment_ids()
            self._aug_src = (self.Xtr, self.Ltr)
            self.Xtr, self.Ltr = torch.empty_like(self.Xtr), torch.empty_like(self.Ltr)
        # train_dynamics: the per-row integer state (ops.train_dynamics_buffers) lives on the net, so that partial_fit / a warm
        # start goes on adding to it; with the option off nothing is allocated and end_epoch queues nothing
        self.dynamics = net._train_dynamics_state(self) if net._train_dynamics_on() else None
        self.epochs_left = int(net.max_epochs)
        self.done = self.epochs_left <= 0

    def begin_epoch(self):
        self.t0 = time.time()

    def lr_table(self):
        """The learning rates of the coming epoch's train batches, in order (None: no schedule, every batch runs at ``net.lr_``).
        Call once per epoch, before any of its work is queued: a scheduler stepped past its end raises here."""
        if self.schedule is None:
            return None
        self.epoch_lrs = self.schedule.epoch_table((self.n_visit + self.bs - 1) // self.bs)
        return self.epoch_lrs

    def order(self):
        """The coming epoch's visit order of the train rows: int64 host array [n_visit], or None (dataset order).  Call once
        per epoch, before any of its work is queued, next to ``lr_table``."""
        self.epoch_order = self.sampler.next_epoch() if self.sampler is not None else None
        self.order_dev = self.y_visit_dev = None
        if self.balance is not None:
            # a balanced epoch's order never exists on the host: drawn on the fit's stream, in front of the epoch's work, into
            # the run's two device tables (order, labels in visit order); with drop_last the epoch visits their full batches
            order, y_visit = self.balance.order(self.ytr, self.net.balance_seed_, len(self.net.history), out=self._bal_out)
            self.set_visit(order[:self.n_visit], y_visit[:self.n_visit])
        if self.augment is not None:
            # the epoch's augmented train rows: a function of (rows, seed, epoch number) per dataset row, queued on the fit's
            # stream in front of the epoch's work (and behind the previous epoch's, which read the same two buffers)
            pad, unk = self._aug_ids
            ops.augment_rows(*self._aug_src, pad, unk, self.augment["frame_drop"], self.augment["token_mask"], self.net.augment_seed_,
                             len(self.net.history), out=(self.Xtr, self.Ltr))
        return self.epoch_order

    def visit_table(self):
        """What a shuffled epoch needs on the device, as one host array int64 [2, n_visit]: the order (range-checked) and the
        labels in visit order -- the epoch's log-probs land at visit position, so that is what train scoring pairs them with."""
        order = sampler.check_order(self.epoch_order, len(self.tr), self.n_visit)
        return np.stack([order, self.tr.y[order].astype(np.int64)])

    def set_visit(self, order_dev, y_visit_dev):
        """The device copies of ``visit_table``'s two rows (uploaded by whoever drives the epoch: one copy per lockstep group)."""
        self.order_dev, self.y_visit_dev = order_dev, y_visit_dev

    def train_labels(self):
        """(device, host) labels of the rows the epoch's train log-probs belong to, in visit order."""
        if self.epoch_order is not None:
            return self.y_visit_dev, self.tr.y[self.epoch_order]
        if self.balance is not None:
            # the one device-to-host copy a balanced epoch adds, taken after the epoch's synchronisation point
            return self.y_visit_dev, self.y_visit_dev.cpu().numpy()
        if self.n_visit != len(self.tr):
            return self.ytr[:self.n_visit], self.tr.y[:self.n_visit]
        return self.ytr, self.tr.y

    def train_labels_dev(self):
        """``train_labels``' device half alone: no host copy is taken (a balanced epoch's labels exist on the device only)."""
        if self.epoch_order is not None or self.balance is not None:
            return self.y_visit_dev
        return self.ytr[:self.n_visit] if self.n_visit != len(self.tr) else self.ytr

    def _reduced_scores(self, names, split, logp, y_dev, y_host):
        """``metrics.epoch_scores`` into this fit's own device buffers for ``split`` (allocated once, not every epoch)."""
        if logp.is_cuda and split not in self._score_out:
            self._score_out[split] = ops.score_buffers(logp.shape[0], logp.shape[1], logp.device)
        if logp.is_cuda and split not in self._rel_out:
            cal = [metrics.calibration_metric_of(n) for n in names]
            self._rel_out[split] = {bins: ops.reliability_buffers(logp.shape[0], bins, logp.device)
                                    for bins in sorted({c[1] or metrics.DEFAULT_BINS for c in cal if c is not None})}
        if logp.is_cuda and split not in self._rank_out and any(n in metrics.RANKING for n in names):
            self._rank_out[split] = ops.ranking_buffers(logp.shape[0], logp.shape[1], logp.device, per_row=False)
        return metrics.epoch_scores(names, logp, y_dev, y_host, split=split, out=self._score_out.get(split),
                                    rel_out=self._rel_out.get(split), rank_out=self._rank_out.get(split))

    def end_epoch(self, tr, va):
        """tr / va: (sample-weighted mean loss, log-probs [n, V] on the device, [(batch loss, batch size)]) of the epoch's
        train and valid passes (va None without a valid split).  Returns True when the fit is over."""
        net = self.net
        tr_loss, tr_logp, tr_batches = tr
        epoch = len(net.history) + 1
        if self.dynamics is not None:
            # the epoch's train log-probs, folded into the per-row state: two launches queued on the fit's stream, no host wait --
            # in front of the history row and of the checkpoint, which saves the state with this epoch in it
            ops.train_dynamics_epoch(tr_logp, self.train_labels_dev(), self.order_dev, epoch, self.dynamics["buf"])
        if self.schedule is not None:
            # what the reference's lr scoring reads at epoch end: with batch stepping the rate after the epoch's last step
            net._set_lr(self.schedule.rates)
        row = {"epoch": epoch, "train_loss": tr_loss, "lr": net.lr_,
               "batches": [{"train_loss": l, "train_batch_size": n} for l, n in tr_batches]}   # skorch history layout
        if self.sampler is not None:
            row["shuffle_seed"] = self.sampler.seed          # a resumed fit rebuilds the order from it (slnlp/sampler.py)
        if self.balance is not None:
            row["balance_seed"] = net.balance_seed_          # with the epoch number, all a resumed fit needs to go on drawing
        if self.augment is not None:
            row["augment_seed"] = net.augment_seed_          # likewise: the draw of epoch e is a function of (rows, seed, e)
        if self.schedule is not None and self.schedule.per_batch:
            for b, lr in zip(row["batches"], self.epoch_lrs):
                b["event_lr"] = lr[0] if isinstance(lr, list) else lr     # the rate this batch used (param groups: group 0's)
        if va is not None:
            va_loss, va_logp, va_batches = va
            row["batches"] += [{"valid_loss": l, "valid_batch_size": n} for l, n in va_batches]
            row["valid_loss"] = va_loss
            row["valid_loss_best"] = bool(va_loss < self.best_valid)
            self.best_valid = min(self.best_valid, va_loss)
        # EpochScoring on the epoch's cached predictions: the reference's five metrics, the macro family, balanced and top-k
        # accuracy from one device-side reduction (slnlp/metrics.py, same numbers as the sklearn scorers); anything else through sklearn
        # (train: paired with the labels in VISIT order, what skorch's cached predictions give EpochScoring under a shuffling loader)
        splits = [("train", tr_logp) + self.train_labels()] + ([("valid", va_logp, self.yva, self.va.y)] if va is not None else [])
        names = [wr.score for wr in self.wrappers]
        fast = {sp: self._reduced_scores(names, sp, lp, yd, yh) if self.fast_ok and names else {} for sp, lp, yd, yh in splits}
        proba = {}
        for wr in self.wrappers:
            for sp, lp, yd, yh in splits:
                if wr.score in fast[sp]:
                    row[f"{sp}_{wr.score}"] = fast[sp][wr.score]
                    continue
                if sp not in proba:
                    proba[sp] = np.exp(lp.cpu().numpy())
                row[f"{sp}_{wr.score}"] = float(wr(_CachedPredictor(proba[sp], net.classes_), None, yh))
        if getattr(net, "_avg_opts", None) is not None:
            row["n_averaged"] = next_n_averaged(net._avg_opts, net.history, len(tr_batches))
        row["dur"] = time.time() - self.t0
        net.history.append(row)
        if net.verbose:
            print("  ".join(f"{k}={v:.4f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items() if k != "batches"))
        if net.checkpoint_dir and row.get("valid_loss_best"):
            net.save_params(net.checkpoint_dir)
        monitor = row.get("valid_loss", tr_loss)
        if self.plateau is not None:                         # LRScheduler(monitor=valid_loss, step_every=epoch)
            self.plateau.step(monitor)
            net._set_lr([g["lr"] for g in self.plateau.optimizer.param_groups] if net._groups else self.plateau.optimizer.param_groups[0]["lr"])
        if self.schedule is not None:                        # LRScheduler(step_every=epoch); a no-op with batch stepping
            self.schedule.epoch_end()
            net._set_lr(self.schedule.rates)
        self.epochs_left -= 1
        if self.es:                                          # skorch EarlyStopping, lower_is_better
            es = self.es
            if monitor < self.dyn_thr:
                self.misses = 0
                thr = float(es.get("threshold", 1e-4))
                self.dyn_thr = monitor - (thr * monitor if es.get("threshold_mode", "rel") == "rel" else thr)
            else:
                self.misses += 1
            if self.misses == int(es.get("patience", 5)):
                if net.verbose:
                    print(f"Stopping since valid_loss has not improved in the last {self.misses} epochs.")
                self.done = True
        if self.epochs_left <= 0:
            self.done = True
        return self.done


class NeuralNetClassifier(LogProbJudge, ClassifierMixin, BaseEstimator):
    _OWN = ("module", "criterion", "optimizer", "lr", "max_epochs", "batch_size", "device", "warm_start", "verbose",
            "predict_nonlinearity", "scoring", "labels", "early_stopping", "gradient_clipping", "lr_scheduler",
            "checkpoint_dir", "train_split", "use_graph", "callbacks", "dataset", "weight_averaging", "calibration", "conformal",
            "train_dynamics")

    def __init__(self, module, criterion="torch.nn.CrossEntropyLoss", optimizer="torch.optim.SGD", lr=0.01,
                 max_epochs=10, batch_size=128, device="cuda", warm_start=False, verbose=0,
                 predict_nonlinearity="auto", scoring=None, labels=None, early_stopping=None,
                 gradient_clipping=None, lr_scheduler=None, checkpoint_dir=None, train_split=5, use_graph="auto",
                 callbacks=None, dataset=None, weight_averaging=None, calibration=None, conformal=None, train_dynamics=False,
                 **kwargs):
        loc = locals()
        self._params = {k: loc[k] for k in self._OWN}
        for k, v in kwargs.items():
            if not any(k.startswith(p) for p in ("module__", "optimizer__", "criterion__", "iterator_train__",
                                                 "iterator_valid__", "callbacks__")):
                raise TypeError(f"NeuralNetClassifier: unexpected argument {k!r}")
            self._params[k] = v
        self.initialized_ = False
        self.history = []
        self._apply_callbacks(callbacks)

    # skorch callback objects (helper.py:197-273 builds Checkpoint, EarlyStopping, GradientNormClipping, LRScheduler and
    # EpochScoring instances) are translated, by class name and public attributes, into the settings this loop
    # implements natively; a callback it cannot honour is an error, never silently dropped.
    _COSMETIC_CALLBACKS = ("PrintLog", "ProgressBar", "EpochTimer", "PassthroughScoring")

    def _apply_callbacks(self, callbacks):
        if callbacks in (None, "disable", []):
            return
        scoring = list(self._params.get("scoring") or [])
        for cb in callbacks:
            obj = cb[1] if isinstance(cb, tuple) else cb
            kind = type(obj).__name__
            get = lambda k, d=None: getattr(obj, k, d)
            if kind == "EarlyStopping":
                if get("monitor", "valid_loss") != "valid_loss" or not get("lower_is_better", True):
                    raise ValueError("EarlyStopping: only monitor='valid_loss', lower_is_better=True is implemented")
                self._params["early_stopping"] = {"patience": get("patience", 5), "threshold": get("threshold", 1e-4),
                                                  "threshold_mode": get("threshold_mode", "rel")}
            elif kind == "GradientNormClipping":
                self._params["gradient_clipping"] = {"gradient_clip_value": get("gradient_clip_value")}
            elif kind == "LRScheduler":
                setting = schedule.from_callback(obj)
                if schedule.is_plateau(setting) and get("monitor", "valid_loss") != "valid_loss":
                    raise ValueError("LRScheduler: ReduceLROnPlateau is implemented on monitor='valid_loss' only")
                if not self._params.get("optimizer__param_groups"):     # (with groups: checked per group in initialize())
                    schedule.check_setting(setting, self._params["lr"])
                self._params["lr_scheduler"] = setting
            elif kind == "Checkpoint":
                if get("monitor", "valid_loss_best") != "valid_loss_best":
                    raise ValueError("Checkpoint: only monitor='valid_loss_best' is implemented")
                self._params["checkpoint_dir"] = get("dirname")
            elif kind == "EpochScoring":
                sc = get("scoring")
                name = sc if isinstance(sc, str) else getattr(sc, "score", None)
                if get("name") == "lr":
                    continue                                  # every history row carries lr already
                if not isinstance(name, str):
                    raise ValueError("EpochScoring: scoring must be a metric name or a ScoringWrapper")
                if name not in scoring:
                    scoring.append(name)                      # both splits are scored for every metric
            elif kind in self._COSMETIC_CALLBACKS:
                continue
            else:
                raise TypeError(f"NeuralNetClassifier: callback {kind!r} has no equivalent in the fused fit loop")
        if scoring:
            self._params["scoring"] = scoring

    # ------------------------------------------------------------ sklearn API
    def get_params(self, deep=True):
        return dict(self._params)

    def set_params(self, **params):
        for k, v in params.items():
            self._params[k] = v
        if params.get("callbacks") is not None:
            self._apply_callbacks(params["callbacks"])
        return self

    def __getattr__(self, name):
        p = self.__dict__.get("_params", {})
        if name in p:
            return p[name]
        raise AttributeError(name)

    def _sub(self, prefix):
        n = len(prefix) + 2
        return {k[n:]: v for k, v in self._params.items() if k.startswith(prefix + "__")}

    # ------------------------------------------------------------- lifecycle
    def _iterator_train(self):
        """(shuffle, drop_last) of the train iterator: the two ``iterator_train__*`` keys the fit loop honours."""
        it = self._sub("iterator_train")
        out = []
        for k in sampler.HONOURED:
            v = it.get(k, False)
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"iterator_train__{k}={v!r}: expected True or False")
            out.append(bool(v))
        return tuple(out)

    def _iterator_train_balance(self):
        """``iterator_train__balance``: class-balanced train epochs drawn on the device (slnlp/sampler.py); default False."""
        v = self._sub("iterator_train").get(sampler.BALANCE, False)
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"iterator_train__{sampler.BALANCE}={v!r}: expected True or False")
        return bool(v)

    def _iterator_train_augment(self):
        """``iterator_train__augment``: {frame_drop, token_mask} with the defaults filled in, or None (off); slnlp/sampler.py."""
        return sampler.augment_options(self._sub("iterator_train").get(sampler.AUGMENT))

    def _augment_ids(self):
        """(pad, unk) of the module's source vocabulary: what fills an augmented row's tail and what a masked token becomes."""
        vocab = self._sub("module").get("src_vocab")
        if vocab is None or not hasattr(vocab, "stoi"):
            raise ValueError("iterator_train__augment: the <pad> and <unk> ids come from the module's source vocabulary, and "
                             f"module__src_vocab is {vocab!r}")
        from model.util import UNK_WORD, get_pad_idx
        return int(get_pad_idx(vocab)), int(vocab.stoi[UNK_WORD])

    def _epoch_rows(self, ds):
        """Rows a train epoch on ``ds`` visits before drop_last: the train split's, or a balanced epoch's."""
        y = ds.y[self._train_split(ds)[0]]
        return sampler.balanced_rows(y) if self._iterator_train_balance() else len(y)

    def _draw_iterator_seeds(self, shuffle, balance, augment=False):
        """``shuffle_seed_`` / ``balance_seed_`` / ``augment_seed_``: each drawn from torch's global CPU generator only when its
        option is on (None otherwise), in this order -- a configuration without an option consumes what it always did."""
        self.shuffle_seed_ = sampler.draw_seed() if shuffle else None
        self.balance_seed_ = sampler.draw_seed() if balance else None
        self.augment_seed_ = sampler.draw_seed() if augment else None

    def initialize(self):
        avg_opts = averaging_options(self._params.get("weight_averaging"))   # a bad setting: here, not in the middle of a fit
        cal_opts = calibration_options(self._params.get("calibration"))
        if cal_opts is not None and not self.train_split:
            raise ValueError(f"calibration: the temperature is fitted on the fit's internal valid split, and train_split={self.train_split!r} "
                             "holds nothing out")
        conf_opts = conformal_options(self._params.get("conformal"))
        if conf_opts is not None and not self.train_split:
            raise ValueError(f"conformal: the threshold is taken on the fit's internal valid split, and train_split={self.train_split!r} "
                             "holds nothing out (conformalize(X, y) takes it on data of yours)")
        if not isinstance(self._params.get("train_dynamics", False), (bool, np.bool_)):
            raise ValueError(f"train_dynamics={self._params['train_dynamics']!r}: expected True or False")
        ok, pairs = optimizer_kwargs(self._sub("optimizer"))
        if not pairs:
            schedule.check_setting(self.lr_scheduler, self.lr)  # a setting the loop cannot honour: here, not in the middle of a fit
        shuffle, _ = self._iterator_train()
        balance = self._iterator_train_balance()
        augment = self._iterator_train_augment()             # a bad setting: here, not in the middle of a fit
        if augment is not None:
            self._augment_ids()
        dev = torch.device(self.device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("slnlp.net: device %r -- the HIP path is the only compute path (no CPU fallback)" % (self.device,))
        kw = self._sub("module")
        kw.setdefault("device", dev)
        self.criterion_ = _resolve(self.criterion)(**self._sub("criterion"))
        if isinstance(self.criterion_, torch.nn.Module):
            self.criterion_ = self.criterion_.to(dev)    # class weights on the device of the torch-stepped path's log-probs
            # (criterion.pt is written from a host copy: save_params)
        self._opt_cls = _resolve(self.optimizer)
        self._opt_kwargs = ok                            # the constructor's keywords; optimizer__param_groups travels apart
        mod_cls = _resolve(self.module)
        # which fused clip + update kernel replaces the torch optimizer (None: the fit steps through torch)
        self._fused_kind = fused_kind(self.criterion_, self._opt_cls, ok, mod_cls, pairs)
        self._fused = self._fused_kind is not None
        if avg_opts is not None and not self._fused:
            raise ValueError("weight_averaging: the average is kept on the device by the fused train step, and this fit steps through "
                             f"torch (optimizer {self._opt_cls.__name__}, criterion {type(self.criterion_).__name__}); it is "
                             "implemented for fused fits only (SGD / Adam / AdamW with CrossEntropyLoss on the model.* modules)")
        self._avg_opts = avg_opts
        self._cal_opts = cal_opts
        self._set_calibration(None)
        self._conf_opts = conf_opts
        self._set_conformal(None)
        self._set_rejection(None)
        self._dyn = None                                 # the training dynamics of an earlier fit do not describe the one to come
        self._opt_defaults = optimizer_defaults(self._opt_cls, {"lr": float(self.lr), **ok}) if self._fused else None
        # the criterion the library evaluates (train and eval forwards): the configured one, on both paths, when it can
        self._crit_opts = criterion_options(self.criterion_) if hasattr(mod_cls, "engine") else None
        # a fused fit may take this host thread's own stream; one that steps through torch kernels stays on the device's shared
        # stream and holds the device exclusively while it runs (see STREAM_MODE above)
        self._stream = device_stream(dev, per_thread=(STREAM_MODE == "thread" and self._fused))
        self._gate = device_gate(dev)
        with torch.cuda.stream(self._stream):            # the weight draw / upload too: nothing of a fit runs on another queue
            self.module_ = mod_cls(**kw).to(dev)
        # optimizer__param_groups: the groups (slnlp/param_groups.py) feed the torch optimizer or the fused update's table
        self._groups = param_groups.build([n for n, _ in self.module_.named_parameters()], pairs) if pairs else None
        if self._groups is not None and all(g.pattern is None for g in self._groups):
            self._groups = None                          # no pattern matched anything: one group with the defaults, as without
        if hasattr(self.module_, "set_train_options"):
            self.module_.set_train_options(criterion=self._crit_opts,
                                           update=update_options(self._fused_kind, self._opt_defaults) if self._fused else None,
                                           param_groups=self._group_table() if self._fused else None)
        if not self._fused:
            what = (param_groups.torch_groups(self._groups, self.module_.named_parameters()) if self._groups is not None
                    else self.module_.parameters())
            self.optimizer_ = self._opt_cls(what, lr=self.lr, **ok)
        self.lr_ = float(self.lr)
        self._set_lr(self._base_lrs())
        if pairs:
            # the schedule's per-group arguments against the real group count -- known only once the module's parameter names
            # are (a pattern that matches nothing makes no group), so with groups this check comes after the module is built
            schedule.check_setting(self.lr_scheduler, self._base_lrs())
        self.history = []
        # the seed of the shuffled order, drawn the way RandomSampler draws one without a generator -- AFTER the module's
        # weights and only when shuffling is on, so the initial weights of every other configuration keep their bits
        self._draw_iterator_seeds(shuffle, balance, augment is not None)
        self.initialized_ = True
        return self

    def _enter_stream(self):
        """Order the fit's stream behind what this thread queued on the ambient stream so far (the weight draw / upload of
        ``initialize``, the dataset upload): ``self._stream`` is a non-blocking stream, nothing else makes it wait."""
        self._stream.wait_stream(torch.cuda.current_stream(self._stream.device))

    def _device_data(self, ds):
        if isinstance(ds, DeviceRows):                       # built on the device (LogProbJudge.attribute): handed on as they are
            return ds.ids, ds.lengths, ds.y
        dev = self.module_._arena.device if hasattr(self.module_, "_arena") else torch.device(self.device)
        return (torch.from_numpy(ds.ids).to(dev), torch.from_numpy(ds.lengths).to(dev), torch.from_numpy(ds.y).to(dev))

    # ------------------------------------------------------------------- fit
    def fit(self, X, y=None, **fit_params):
        if not (self.warm_start and self.initialized_):
            self.initialize()
        return self.partial_fit(X, y, **fit_params)

    def partial_fit(self, X, y=None, **fit_params):
        if not self.initialized_:
            self.initialize()
        self._gate.enter(not self._fused)
        try:
            return self._partial_fit_gated(X, y)
        finally:
            self._gate.leave(not self._fused)

    def _partial_fit_gated(self, X, y):
        self._enter_stream()
        if getattr(self, "_cal_opts", None) is not None:
            self._set_calibration(None)                      # an earlier fit's temperature does not describe the weights to come
        if getattr(self, "_conf_opts", None) is not None:
            self._set_conformal(None)                        # nor does its threshold
        self._set_rejection(None)                            # nor a rejection threshold taken with fit_rejection
        with torch.cuda.stream(self._stream):
            run = _FitRun(self, self._as_dataset(X, y))
            for _ in range(int(self.max_epochs)):
                run.begin_epoch()
                self.module_.train()
                lrs, order = run.lr_table(), run.order()
                if order is not None:                       # one upload per epoch: the order and the labels in visit order
                    # (a balanced epoch has no host order: run.order() drew its tables on the device)
                    run.set_visit(*torch.from_numpy(run.visit_table()).to(run.Xtr.device))
                averaging = self._averaging_epoch()
                if self._avg_opts is not None and self._avg_opts["every"] == "batch":
                    # the accumulator's launches ride every train step from start_epoch on: switched between epochs, once
                    self.module_.set_averaging(*((self._avg_opts["kind"], self._avg_opts["decay"]) if averaging else (None,)))
                tr = self._run_epoch(run.Xtr, run.Ltr, run.ytr, run.bs, True, run.momentum, run.max_norm, lrs=lrs,
                                     order=run.order_dev, n_visit=run.n_visit)
                if averaging and self._avg_opts["every"] == "epoch":
                    # behind the epoch's last step, in front of the valid pass (which reads the live weights), on the fit's stream
                    self.module_.average_now(self._avg_opts["kind"], self._avg_opts["decay"])
                va = None
                if run.va is not None:
                    self.module_.eval()
                    va = self._run_epoch(run.Xva, run.Lva, run.yva, run.bs, False, run.momentum, run.max_norm)
                if run.end_epoch(tr, va):
                    break
            logp = self._calibrate(run) if getattr(self, "_cal_opts", None) is not None else None
            if getattr(self, "_conf_opts", None) is not None:
                self._conformalize_fit(run, logp)
        stream_sync(self._stream)
        return self

    # ------------------------------------------------------------ calibration
    def _calibrate(self, run):
        """Fit the temperature on the valid split's log-probs under the weights ``predict_proba`` evaluates with (the averaged
        ones swapped in and back, as there); the [N, V] matrix stays on the device, only the state comes to the host."""
        if run.va is None:
            raise ValueError("calibration: the fit has no valid split to fit the temperature on (train_split)")
        logp = self._valid_logp(run)
        self._set_calibration(*download_calibration(self._cal_opts, fit_calibration(self._cal_opts, logp, run.yva)))
        return logp

    def _valid_logp(self, run):
        """The valid split's device log-probs under the weights ``predict_proba`` evaluates with."""
        self.module_.eval()
        swapped = self._predict_averaged()
        if swapped:
            self.module_.swap_averaged()
        try:
            return self._run_epoch(run.Xva, run.Lva, run.yva, run.bs, False, run.momentum, run.max_norm)[1]
        finally:
            if swapped:
                self.module_.swap_averaged()

    def _set_calibration(self, info, state=None, bias=None):
        """``calibration_`` (``ops.temperature_download``'s dict, or ``ops.bias_temperature_download``'s), ``temperature_`` and the
        device state -- and, for a ``bias_temperature`` fit, the device bias -- ``predict_proba`` calibrates with; None removes
        them.  A fit that cannot stand raises here: labels outside the classes, the temperature search's iteration cap.  A
        ``bias_temperature`` fit that ends at its evaluation cap or on a non-positive pivot stands -- every accepted step lowered
        the objective -- and warns."""
        if info is None:
            for k in ("calibration_", "temperature_", "_cal_state", "_cal_bias"):
                self.__dict__.pop(k, None)
            return
        if info["bad_labels"] > 0:
            raise ValueError(f"calibrating on the valid data: {info['bad_labels']} of {info['rows'] + info['bad_labels']} labels lie "
                             "outside the classes of the log-probs")
        dev = self.module_._arena.device if hasattr(self.module_, "_arena") else torch.device(self.device)
        if info.get("method") == "bias_temperature":
            if info["reason"] in ("cap", "pivot"):
                warnings.warn(f"calibration: the bias_temperature search ended with reason {info['reason']!r} after {info['iterations']} "
                              f"evaluations (beta {info['beta']!r}): the result is the last accepted point, not a converged one",
                              RuntimeWarning, stacklevel=3)
            if state is None:
                state, bias = ops.bias_temperature_state(info["beta"], info["bias"], dev)
            self._cal_state, self._cal_bias = state, bias
            self.calibration_, self.temperature_ = dict(info), info["temperature"]
            return
        if info["reason"] == "cap":
            raise RuntimeError(f"calibration: the temperature search did not converge in {info['iterations']} iterations "
                               f"(beta {info['beta']!r})")
        self.__dict__.pop("_cal_bias", None)
        self._cal_state = state if state is not None else ops.temperature_state(info["beta"], dev)
        self.calibration_, self.temperature_ = dict(info), info["temperature"]

    # ------------------------------------------------------ conformal sets
    def _conformalize_fit(self, run, logp=None):
        """The ``conformal`` option at the end of a fit: the threshold on the valid split's log-probs (``logp``: those the
        temperature was just fitted on; None: a forward pass under the weights ``predict_proba`` uses), at the fit's
        temperature when it has one.  This split also chose the temperature and the stopping epoch, so the 1 - alpha guarantee
        is approximate here; it is exact only with ``conformalize`` on rows the fit never saw."""
        if run.va is None:
            raise ValueError("conformal: the fit has no valid split to take the threshold on (train_split)")
        if logp is None:
            logp = self._valid_logp(run)
        self._set_conformal(self._conf_opts, *self._conformal_calibrate(logp, run.yva, self._conf_opts, True), labels=run.va.y,
                            where="the valid data")

    # ------------------------------------------------------- weight averaging
    def _averaging_epoch(self):
        """Whether the epoch about to run feeds the average (the option is on and ``start_epoch`` is reached)."""
        av = getattr(self, "_avg_opts", None)
        return av is not None and len(self.history) + 1 >= av["start_epoch"]

    @property
    def n_averaged_(self):
        """Models in the running average, from the history (no device read)."""
        return int(self.history[-1].get("n_averaged", 0)) if self.history else 0

    def _predict_averaged(self):
        av = getattr(self, "_avg_opts", None)
        return av is not None and av["predict"] and self.n_averaged_ > 0

    def averaged_state_dict(self):
        """The module's ``state_dict`` with every parameter replaced by its running average (buffers as they are)."""
        if getattr(self, "_avg_opts", None) is None:
            raise RuntimeError("averaged_state_dict: this estimator has no weight_averaging option")
        sd = dict(self.module_.state_dict())
        avg = self.module_.averaged_arena()[0]
        for name, shape, off in self.module_._entries:
            n = 1
            for d in shape:
                n *= d
            sd[name] = avg[off:off + n].view(*shape).clone()
        return sd

    def _train_split(self, ds):
        ts = self.train_split
        if not ts:
            return np.arange(len(ds)), None
        if getattr(ds, "groups", None) is not None:          # near-duplicate groups stay on one side: slnlp/data.py
            from .data import group_folds
            return group_folds("NeuralNetClassifier", "train_split", ds.y, ds.groups, int(ts))[0]
        from sklearn.model_selection import KFold, StratifiedKFold
        idx = np.arange(len(ds))
        try:
            tr, va = next(iter(StratifiedKFold(n_splits=int(ts)).split(idx, ds.y)))
        except ValueError:                                   # a class with fewer members than folds
            tr, va = next(iter(KFold(n_splits=int(ts)).split(idx)))
        return tr, va

    def _base_lrs(self):
        """The configured rate: ``lr``, or with param groups the list of every group's (its own ``lr``, else ``lr``)."""
        if getattr(self, "_groups", None) is None:
            return float(self.lr)
        return param_groups.resolved(self._groups, {"lr": self.lr}, "lr")

    def _group_table(self):
        """The fused update's device table of the groups (False: none), for ``module_.set_train_options``."""
        if self._groups is None:
            return False
        begin, group = param_groups.segments(self._groups, self.module_._entries, self.module_._arena.numel())
        return {"seg_begin": begin, "seg_group": group,
                "weight_decay": param_groups.resolved(self._groups, self._opt_defaults, "weight_decay")}

    @property
    def lrs_(self):
        """The current rate of every param group (``lr_`` is group 0's, what the history's ``lr`` records)."""
        return list(self._lrs) if getattr(self, "_groups", None) is not None else [self.lr_]

    def _set_lr(self, lr):
        """``lr``: one rate, or with param groups the list of the groups' rates."""
        if getattr(self, "_groups", None) is not None:
            if not isinstance(lr, (list, tuple)) or len(lr) != len(self._groups):
                raise ValueError(f"_set_lr: {len(self._groups)} param groups need a list of {len(self._groups)} rates, got {lr!r}")
            self._lrs = [float(v) for v in lr]
            self.lr_ = self._lrs[0]
            if not self._fused:
                for g, v in zip(self.optimizer_.param_groups, self._lrs):
                    g["lr"] = v
            return
        self.lr_ = float(lr)
        if not self._fused:
            for g in self.optimizer_.param_groups:
                g["lr"] = self.lr_

    def _run_epoch(self, X, L, y, bs, train, momentum, max_norm, lrs=None, order=None, n_visit=None):
        """One pass in dataset order, or -- ``order``: int64 device tensor [n_visit] -- over rows ``order[0], order[1], ...``
        (a shuffled train epoch: every batch is staged by the library's gather launch, whichever way the fit steps, so no
        torch indexing kernel joins the stream); ``n_visit``: rows visited (None: all; fewer with drop_last).  ``lrs``: the
        learning rate of each train batch (``_FitRun.lr_table``; None: ``lr_`` throughout).  Returns (sample-weighted mean
        loss, log-probs [n_visit, V] on the device in visit order, [(batch loss, batch size)])."""
        n = X.shape[0] if n_visit is None else int(n_visit)
        losses, sizes, outs = [], [], []
        for k, i in enumerate(range(0, n, bs)):
            stop = min(i + bs, n)
            if order is not None:
                # fused fits gather straight into their plan's fixed staging buffers (the ones a captured graph reads)
                stage = self.module_.engine(stop - i, X.shape[1]).staging() if train and self._fused else None
                xb, lb, yb = ops.gather_batch(X, L, y, order, i, stop - i, out=stage)
            else:
                xb, lb, yb = X[i:stop], L[i:stop], y[i:stop]
            if train and lrs is not None:
                self._set_lr(lrs[k])                        # one schedule for the fused and the torch-stepped path
            if train and self._fused:
                eng = self.module_.engine(xb.shape[0], xb.shape[1])
                eng.set_lr(self.lr_)
                if self._groups is not None:
                    self.module_.set_group_lrs(self._lrs)    # what the grouped update reads instead
                if self._fused_kind in ("adam", "adamw"):
                    betas, eps, wd = adam_args(self)
                    logp = eng.train_step_adam(xb, yb, self.module_.adam_second_moment(), betas, eps, wd, max_norm, lengths=lb)
                else:
                    logp = eng.step(xb, yb, lb, momentum, max_norm, graph=self.use_graph if self.use_graph == "auto" else bool(self.use_graph))
                losses.append(eng.scalars[0].clone())
            elif train:
                self.optimizer_.zero_grad()
                logp = self.module_(X=xb, y=yb, lengths=lb)
                loss = self.criterion_(logp, yb)
                loss.backward()
                if max_norm:
                    torch.nn.utils.clip_grad_norm_(self.module_.parameters(), max_norm)
                self.optimizer_.step()
                losses.append(loss.detach())
            else:
                with torch.no_grad():
                    logp = self.module_(X=xb, y=yb, lengths=lb)
                    if hasattr(self.module_, "engine") and self._crit_opts is not None:
                        losses.append(self.module_.engine(xb.shape[0], xb.shape[1]).scalars[0].clone())
                    else:
                        losses.append(self.criterion_(logp, yb))
            sizes.append(xb.shape[0])
            outs.append(logp.detach().clone())
        per_batch = torch.stack(losses).float().cpu()                       # one sync per epoch
        w = torch.tensor(sizes, dtype=torch.float32)
        mean = float((per_batch * w).sum() / w.sum())
        return mean, torch.cat(outs), list(zip(per_batch.tolist(), sizes))

    # --------------------------------------------------------------- predict
    def _forward_logp(self, ds, then):
        """The module's float32 log-probs [len(ds), V] of ``ds`` on the device -- the forward passes of ``predict_proba``: under
        the gate, on the fit's stream, the averaged weights swapped in where the fit predicts with them and back afterwards --
        handed, still on that stream, to ``then(logp, y_dev)``; returns what ``then`` returns once the stream has drained."""
        self.module_.eval()
        outs = []
        self._gate.enter(not self._fused)
        try:
            self._enter_stream()
            with torch.cuda.stream(self._stream), torch.no_grad():
                Xd, Ld, yd = self._device_data(ds)
                swapped = self._predict_averaged()
                if swapped:
                    self.module_.swap_averaged()         # the averaged weights stand in for the forward passes ...
                try:
                    for i in range(0, len(ds), int(self.batch_size)):
                        outs.append(self.module_(X=Xd[i:i + self.batch_size], y=yd[i:i + self.batch_size], lengths=Ld[i:i + self.batch_size]))
                finally:
                    if swapped:
                        self.module_.swap_averaged()     # ... and the live weights come back bit for bit
                res = then(torch.cat(outs), yd)
            stream_sync(self._stream)
        finally:
            self._gate.leave(not self._fused)
        return res

    # ------------------------------------------------------------ checkpoint
    def _sgd_state_dict(self):
        """The fused update's momentum arena as a ``torch.optim.SGD.state_dict()``: one ``momentum_buffer`` per parameter,
        in ``module.parameters()`` order, plus the param group with the current lr -- what skorch's Checkpoint writes as
        optimizer.pt (helper.py:211-213) and what ``torch.optim.SGD.load_state_dict`` reads back."""
        params = dict(self.module_.named_parameters())
        if self._groups is not None:
            # the same groups the torch-stepped path would build: torch numbers the state by position across them
            opt = self._opt_cls(param_groups.torch_groups(self._groups, params.items()), lr=float(self.lr), **self._opt_kwargs)
            for g, v in zip(opt.param_groups, self._lrs):
                g["lr"] = v
        else:
            opt = self._opt_cls([p for n, p in params.items()], lr=self.lr_, **self._opt_kwargs)
        st = self.module_._shared_state()
        mom = st["momentum"]
        adam = self._fused_kind in ("adam", "adamw")
        # torch.optim.SGD keeps no momentum buffer before its first step (the first-step rule of dampening reads that): the
        # library's SGD step count (scalars[3]) says whether there was one
        sgd_started = adam or float(st["scalars"][3]) > 0
        step = None
        if adam:
            step = float(st["scalars"][2])
            v2 = self.module_.adam_second_moment()
        for name, shape, off in self.module_._entries:
            if name in self.module_._dead_params:
                continue                                   # never receives a gradient: torch keeps no state for it
            n = 1
            for d in shape:
                n *= d
            view = lambda arena: arena[off:off + n].view(*shape).detach().cpu().clone()
            if adam:
                opt.state[params[name]].update(step=torch.tensor(step), exp_avg=view(mom), exp_avg_sq=view(v2))
            elif sgd_started:
                opt.state[params[name]]["momentum_buffer"] = view(mom)
        return opt.state_dict()

    def _load_sgd_state_dict(self, sd):
        groups = sd.get("param_groups") or [{}]
        if self._groups is not None and (len(groups) != len(self._groups) or
                                         [len(g.get("params", ())) for g in groups] != [len(g.names) for g in self._groups]):
            raise ValueError(f"optimizer.pt holds {len(groups)} param groups that are not this estimator's {len(self._groups)}: "
                             "load it with the optimizer__param_groups it was written with")
        # torch numbers the state by position across the param groups, in group order
        names = param_groups.positions(self._groups) if self._groups is not None else [n for n, _ in self.module_.named_parameters()]
        ent = {n: (shape, off) for n, shape, off in self.module_._entries}
        st = self.module_._shared_state()
        step = None
        started = False
        for idx, state in sd.get("state", {}).items():
            shape, off = ent[names[int(idx)]]
            buf = state.get("momentum_buffer", state.get("exp_avg"))
            started = started or state.get("momentum_buffer") is not None
            if buf is not None:
                st["momentum"][off:off + buf.numel()].copy_(buf.reshape(-1).to(st["momentum"].device, torch.float32))
            if state.get("exp_avg_sq") is not None:
                v2 = self.module_.adam_second_moment()
                v2[off:off + buf.numel()].copy_(state["exp_avg_sq"].reshape(-1).to(v2.device, torch.float32))
                step = float(state.get("step", 0.0))
        if step is not None:                           # the device-side Adam step count (shared by every plan of the module)
            st["scalars"][2] = step
        if self._fused_kind == "sgd":                  # SGD: whether the first step (no dampening) is behind us
            st["scalars"][3] = 1.0 if started else 0.0
        if self._groups is not None:
            self._set_lr([g["lr"] for g in groups])
        elif "lr" in groups[0]:
            self._set_lr(groups[0]["lr"])

    # ------------------------------------------------------- training dynamics
    def _train_dynamics_on(self):
        return bool(self.__dict__.get("_params", {}).get("train_dynamics", False))

    def _train_dynamics_state(self, run):
        """The per-row state a ``train_dynamics=True`` fit adds to (``_FitRun.__init__``): new and reset, or -- ``partial_fit`` / a
        warm start / a loaded checkpoint -- the one this net already holds for the same train rows.  {buf:
        ``ops.train_dynamics_buffers``' dict, idx_tr: the train split's dataset indices, y: its labels}.  Runs on the fit's stream."""
        idx = np.asarray(run.idx_tr, dtype=np.int64)
        dev, N, n_visit = run.ytr.device, len(run.tr), int(run.n_visit)
        dyn = getattr(self, "_dyn", None)
        if dyn is not None and not np.array_equal(dyn["idx_tr"], idx):
            raise ValueError(f"train_dynamics: the state describes {len(dyn['idx_tr'])} train rows of an earlier fit and this fit's train "
                             f"split has {len(idx)} rows with other dataset indices; initialize() (or fit without warm_start) starts anew")
        if dyn is not None and dyn["buf"]["shape"] == (N, n_visit) and dyn["buf"]["flat"].device == dev:
            return dyn
        buf = ops.train_dynamics_buffers(N, n_visit, dev)
        words = buf["state_bytes"] // 4
        if dyn is None:
            ops.train_dynamics_reset(buf)
        else:                                                # the epoch length changed between two partial fits (or the state came
            buf["flat"][:words].copy_(dyn["buf"]["flat"][:words])       # from a checkpoint, which does not know it): the state moves
        self._dyn = {"buf": buf, "idx_tr": idx, "y": np.asarray(run.tr.y).astype(np.int64)}
        return self._dyn

    def train_dynamics(self, top=50, per_row=False):
        """What happened to every row of the fit's train split DURING training (``train_dynamics=True``): dataset cartography
        (Swayamdipta et al. 2020), forgetting events (Toneva et al. 2019) and the area under the margin (Pleiss et al. 2020), kept
        on the device epoch by epoch from the train pass's own log-probs (csrc/train_dynamics.hip: all per-row state is integer,
        so the numbers are a pure function of the fit) -- no extra forward pass, ONE download here.
        ``metrics.train_dynamics_report``'s dict: ``hard`` / ``ambiguous`` / ``forgotten`` / ``low_aum`` (at most ``top`` rows
        each) and ``never_learned``, whose ``row`` entries are indices into the dataset the fit was given and whose ``label``
        entries are ``classes_`` entries; the totals; ``per_class``; plus ``classes``.  ``per_row=True`` keeps ``per_row``, the
        arrays over all train rows.  Unlike ``label_issues`` it is honest on the fit's own train rows by construction: what it
        measures is the memorisation itself.

        The probabilities are the TRAINING pass's: dropout on, augmented inputs under ``iterator_train__augment``, and every
        visit under the weights of its own step (an epoch's first batch saw older weights than its last).  Under
        ``iterator_train__balance`` a row is visited several times per epoch (or not at all), and forgetting is epoch-granular:
        a row counts as right in an epoch when it was right at EVERY visit of it, and an epoch that does not visit it leaves
        its record alone.  For the reference Transformer, whose decoder is fed the gold label, the statistics are conditional
        on that label -- the caveat of ``label_issues`` and ``attribute``.  Raises when the option was off or no epoch has run."""
        if not self._train_dynamics_on():
            raise ValueError("train_dynamics: the estimator was built with train_dynamics=False, nothing was recorded")
        dyn = self.__dict__.get("_dyn")
        if dyn is None:
            raise ValueError("train_dynamics: no epoch has run yet (fit first)")
        got = ops.train_dynamics_download(dyn["buf"])
        if int(got["head"][0]) < 1:
            raise ValueError("train_dynamics: no epoch has run yet (fit first)")
        classes = self.__dict__.get("classes_")              # (a state loaded from a checkpoint, no fit yet: the class ids themselves)
        res = metrics.train_dynamics_report(got, dyn["y"] if classes is None else classes[dyn["y"]], rows=dyn["idx_tr"], top=top)
        res["classes"] = classes
        if not per_row:
            del res["per_row"]
        return res

    def save_params(self, dirname):
        """skorch ``Checkpoint`` artefacts: params.pt (state_dict), optimizer.pt (a torch.optim state_dict in either
        mode), criterion.pt, history.json; calibration.json, conformal.json and rejection.json when the fit has a temperature / a conformal threshold /
        a rejection threshold; train_dynamics.npz (the integer state with its head, the train split's dataset indices and labels)
        when the fit keeps training dynamics."""
        os.makedirs(dirname, exist_ok=True)
        torch.save({k: v.detach().cpu() for k, v in self.module_.state_dict().items()}, os.path.join(dirname, "params.pt"))
        torch.save(self._sgd_state_dict() if self._fused else self.optimizer_.state_dict(), os.path.join(dirname, "optimizer.pt"))
        torch.save({k: v.detach().cpu() if torch.is_tensor(v) else v for k, v in self.criterion_.state_dict().items()},
                   os.path.join(dirname, "criterion.pt"))       # host tensors, like params.pt
        with open(os.path.join(dirname, "history.json"), "w") as f:
            json.dump(self.history, f, indent=1)
        if getattr(self, "calibration_", None) is not None:
            with open(os.path.join(dirname, "calibration.json"), "w") as f:
                json.dump(calibration_to_json(self.calibration_), f, indent=1)
        if getattr(self, "conformal_", None) is not None:
            with open(os.path.join(dirname, "conformal.json"), "w") as f:
                json.dump(self.conformal_, f, indent=1)      # (an infinite qhat is written as Infinity, which json.load reads back)
        if getattr(self, "rejection_", None) is not None:
            with open(os.path.join(dirname, "rejection.json"), "w") as f:
                json.dump(self.rejection_, f, indent=1)      # (repr round-trips the threshold bit for bit; Infinity and NaN as above)
        if self.__dict__.get("_dyn") is not None:         # the training dynamics so far: a resumed fit goes on adding to them
            buf = self._dyn["buf"]                       # (one device-to-host copy of the state's 4-byte words)
            np.savez(os.path.join(dirname, "train_dynamics.npz"), state=buf["flat"][:buf["state_bytes"] // 4].cpu().numpy(),
                     idx_tr=self._dyn["idx_tr"], y=self._dyn["y"])
        if getattr(self, "_avg_opts", None) is not None:  # the running average and how many models it holds: a resumed fit goes on
            torch.save({"state_dict": {k: v.detach().cpu() for k, v in self.averaged_state_dict().items()}, "n_averaged": self.n_averaged_},
                       os.path.join(dirname, "averaged.pt"))

    def load_params(self, dirname):
        """Restore what ``save_params`` / skorch's Checkpoint wrote: weights, optimizer state (momentum buffers + lr) and,
        when present, the history -- training resumes where the checkpoint was taken."""
        if not self.initialized_:
            self.initialize()
        self.module_.load_state_dict(torch.load(os.path.join(dirname, "params.pt")))
        opt_file = os.path.join(dirname, "optimizer.pt")
        if os.path.exists(opt_file):
            sd = torch.load(opt_file)
            if self._fused:
                self._load_sgd_state_dict(sd)
            else:
                self.optimizer_.load_state_dict(sd)
                self.lr_ = float(self.optimizer_.param_groups[0]["lr"])
                if self._groups is not None:
                    self._lrs = [float(g["lr"]) for g in self.optimizer_.param_groups]
        avg_file = os.path.join(dirname, "averaged.pt")
        if getattr(self, "_avg_opts", None) is not None and os.path.exists(avg_file):
            saved = torch.load(avg_file)
            avg, count = self.module_.averaged_arena()
            for name, shape, off in self.module_._entries:
                t = saved["state_dict"][name]
                avg[off:off + t.numel()].copy_(t.reshape(-1).to(avg.device, torch.float32))
            count.fill_(float(saved["n_averaged"]))
        cal_file = os.path.join(dirname, "calibration.json")
        if getattr(self, "_cal_opts", None) is not None and os.path.exists(cal_file):
            with open(cal_file) as f:
                self._set_calibration(calibration_from_json(json.load(f)))      # beta (and the bias) go back to the device
        conf_file = os.path.join(dirname, "conformal.json")
        if os.path.exists(conf_file):
            with open(conf_file) as f:
                info = json.load(f)
            self._set_conformal(conformal_options({k: info[k] for k in CONFORMAL_DEFAULTS}), info=info)     # qhat goes back to the device
        rej_file = os.path.join(dirname, "rejection.json")
        if os.path.exists(rej_file):
            with open(rej_file) as f:
                self._set_rejection(json.load(f))            # the threshold goes back to the device
        dyn_file = os.path.join(dirname, "train_dynamics.npz")
        if self._train_dynamics_on() and os.path.exists(dyn_file):
            with np.load(dyn_file) as saved:             # the integers go back to the device; the fit that continues them checks
                words, idx, y = saved["state"], saved["idx_tr"].astype(np.int64), saved["y"].astype(np.int64)       # its train rows
            dev = self.module_._arena.device if hasattr(self.module_, "_arena") else torch.device(self.device)
            buf = ops.train_dynamics_buffers(len(idx), len(idx), dev)       # (the epoch length is the next fit's to say)
            if words.dtype != np.int32 or words.shape != (buf["state_bytes"] // 4,):
                raise ValueError(f"{dyn_file}: a state of {words.dtype} {words.shape}, {len(idx)} train rows take int32 "
                                 f"({buf['state_bytes'] // 4},)")
            buf["flat"][:words.size].copy_(torch.from_numpy(words))
            self._dyn = {"buf": buf, "idx_tr": idx, "y": y}
        hist = os.path.join(dirname, "history.json")
        if os.path.exists(hist):
            with open(hist) as f:
                self.history = json.load(f)
            seed = sampler.seed_from_history(self.history)
            if seed is not None:                         # the resumed fit continues the checkpoint's order (slnlp/sampler.py)
                self.shuffle_seed_ = seed
            seed = sampler.seed_of(self.history, "balance_seed")
            if seed is not None:                         # ... and the checkpoint's balanced draws, at epoch len(history)
                self.balance_seed_ = seed
            seed = sampler.seed_of(self.history, "augment_seed")
            if seed is not None:                         # ... and its augmentation draws, likewise
                self.augment_seed_ = seed
        return self
