"""Learning-rate schedules of a fit: any ``torch.optim.lr_scheduler`` class, stepped per epoch or per batch.

skorch's ``LRScheduler`` callback takes a policy (a name in ``torch.optim.lr_scheduler`` or the class), ``step_every`` and the
policy's keyword arguments (the reference configures ``ReduceLROnPlateau``, helper.py:226-238).  ``LRSchedule`` is that for
the fused fit loop: it owns a dummy optimizer (one zero parameter per param group, ``lr`` = the estimator's, or each group's
base rate with ``optimizer__param_groups``) and a real scheduler instance on it, so every value is torch's own arithmetic -- nothing is restated in closed form.  The loop asks it for the rates of an
epoch's train batches ahead of the epoch (``epoch_table``), because a lockstep unit runs the whole epoch without coming back
to the host: per-batch rates travel to the device as a table (slnlp.lockstep).

``ReduceLROnPlateau`` is not handled here: it needs the epoch's ``valid_loss`` and keeps its code path in ``slnlp.net._FitRun``.

The position of a schedule is a function of the fit's history: a new fit run builds the schedule from scratch and replays the
steps the history accounts for (``fast_forward``), so a resumed fit needs no extra checkpoint file.
"""
import inspect

import torch
from torch.optim import lr_scheduler as _S

PLATEAU = "ReduceLROnPlateau"
STEP_EVERY = ("epoch", "batch")
# keys of the ``lr_scheduler`` dict that are not the policy's keyword arguments (``monitor`` only means something to the plateau)
_OWN_KEYS = ("policy", "step_every", "monitor")

ACCEPTED = ("accepted: policy = 'ReduceLROnPlateau' (on valid_loss, stepped per epoch), or the name of any other scheduler class "
            "in torch.optim.lr_scheduler (StepLR, MultiStepLR, ExponentialLR, CosineAnnealingLR, CosineAnnealingWarmRestarts, "
            "LinearLR, ConstantLR, PolynomialLR, LambdaLR, CyclicLR, OneCycleLR, ...) or such a class itself; "
            "step_every = 'epoch' (default) | 'batch'; every other key is a keyword argument of the policy")

_BASE = getattr(_S, "LRScheduler", None) or getattr(_S, "_LRScheduler")


def policy_name(policy):
    return policy if isinstance(policy, str) else getattr(policy, "__name__", str(policy))


def is_plateau(setting):
    return policy_name(setting.get("policy", PLATEAU)) == PLATEAU


def from_callback(cb):
    """The ``lr_scheduler`` dict of a skorch-style ``LRScheduler`` callback object (``policy``, ``step_every``, ``kwargs``)."""
    pol = getattr(cb, "policy", PLATEAU)
    kwargs = dict(getattr(cb, "kwargs", None) or {})
    if policy_name(pol) == PLATEAU:
        return {"policy": PLATEAU, **kwargs}               # stepped per epoch whatever the callback says, as before
    return {"policy": pol, "step_every": getattr(cb, "step_every", "epoch"), **kwargs}


def _resolve_policy(policy):
    name = policy_name(policy)
    if name == "WarmRestartLR":
        raise ValueError("lr_scheduler: skorch's WarmRestartLR is not implemented -- use torch's CosineAnnealingWarmRestarts; " + ACCEPTED)
    cls = getattr(_S, policy, None) if isinstance(policy, str) else policy
    if not (inspect.isclass(cls) and issubclass(cls, _BASE)):
        raise ValueError(f"lr_scheduler: policy {policy!r} is not a torch.optim.lr_scheduler class; " + ACCEPTED)
    return cls


class LRSchedule:
    """One fit's schedule.  ``current`` is the rate the next train batch uses (group 0's with param groups, what the history's
    ``lr`` and ``event_lr`` record); ``lr`` a list of G base rates: one dummy group each, ``current_all`` and the rows of
    ``epoch_table`` are then lists of G rates, every one torch's own for that group (per-group ``max_lr`` lists,
    ``lr_lambda`` lists, ... included)."""

    def __init__(self, policy, lr, step_every="epoch", **kwargs):
        if step_every not in STEP_EVERY:
            raise ValueError(f"lr_scheduler: step_every={step_every!r}; " + ACCEPTED)
        cls = _resolve_policy(policy)
        cyc = inspect.signature(cls.__init__).parameters.get("cycle_momentum")
        if cyc is not None and kwargs.get("cycle_momentum", cyc.default):
            # momentum is baked by value into recorded lockstep programs and captured graphs: it cannot follow a cycle, and
            # dropping the request silently would train something else than asked for
            raise ValueError(f"lr_scheduler: {cls.__name__} cycles the momentum by default, which the fused update does not implement "
                             f"-- pass cycle_momentum=False")
        self.policy, self.step_every, self.kwargs = cls, step_every, dict(kwargs)
        self.grouped = isinstance(lr, (list, tuple))
        base = [float(v) for v in lr] if self.grouped else [float(lr)]
        self._opt = torch.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": v} for v in base], lr=base[0])
        try:
            self._sched = cls(self._opt, **kwargs)
        except Exception as e:
            raise ValueError(f"lr_scheduler: cannot construct {cls.__name__}(optimizer, **{kwargs!r}): {type(e).__name__}: {e}; "
                             + ACCEPTED) from e

    @classmethod
    def from_setting(cls, setting, lr):
        """From the estimator's ``lr_scheduler`` dict (not the plateau's)."""
        return cls(setting["policy"], lr, setting.get("step_every", "epoch"),
                   **{k: v for k, v in setting.items() if k not in _OWN_KEYS})

    @property
    def per_batch(self):
        return self.step_every == "batch"

    @property
    def current(self):
        return float(self._opt.param_groups[0]["lr"])

    @property
    def current_all(self):
        return [float(g["lr"]) for g in self._opt.param_groups]

    @property
    def rates(self):
        """What the estimator's ``_set_lr`` takes: ``current``, or with param groups ``current_all``."""
        return self._row()

    def _row(self):
        return self.current_all if self.grouped else self.current

    def _step(self):                                       # skorch: optimizer.step() per batch, then the scheduler
        self._opt.step()
        self._sched.step()

    def epoch_table(self, n):
        """The rates of the next ``n`` train batches (Python floats; with param groups a list of G floats each).  Per-batch stepping advances the scheduler by ``n``
        (a scheduler stepped past its end raises torch's own error here, before anything is queued); per-epoch stepping
        returns ``n`` copies of the current value and leaves the advance to ``epoch_end``."""
        if not self.per_batch:
            return [self._row() for _ in range(n)]
        out = []
        for _ in range(n):
            out.append(self._row())
            self._step()
        return out

    def epoch_end(self):
        if not self.per_batch:
            self._step()

    def fast_forward(self, history):
        """Replay the steps ``history`` (skorch layout: one row per epoch, ``batches`` inside) accounts for."""
        if self.per_batch:
            n = sum(1 for row in history for b in row.get("batches", ()) if "train_loss" in b)
        else:
            n = len(history)
        for _ in range(n):
            self._step()
        return self


def check_setting(setting, lr):
    """Raise ValueError for an ``lr_scheduler`` setting the fit loop cannot honour (where the setting is given, not in the
    middle of a fit)."""
    if not setting:
        return
    if not isinstance(setting, dict):
        raise ValueError(f"lr_scheduler: expected a dict, got {type(setting).__name__}; " + ACCEPTED)
    if is_plateau(setting):
        return                                             # constructed by the fit run, as before
    LRSchedule.from_setting(setting, lr)
