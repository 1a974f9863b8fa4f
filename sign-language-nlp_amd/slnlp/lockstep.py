"""K fits of one shape advancing in lockstep through ONE launch sequence (libslnlp ``slnlp_tf_lockstep_*`` /
``slnlp_rnn_lockstep_*``).

The reference runs the (candidate x fold) fits of its grid one at a time per worker
(/root/reference/main.py:70-78, helper.py:490-526).  One batch-50 fit cannot fill an MI355X -- its decoder stages
are 50-row kernels -- and fits on separate streams only reach 1.26x.  Fits of one work unit (same shapes; own
weights, lr, dropout rate, seed and data) therefore share every kernel launch: a 50-row stage becomes a K x 50-row
stage at the same latency, the grouped GEMM launches carry K times the tiles.  Each fit's arithmetic is untouched,
so its history, weights and scores are bit-identical to a solo fit (tests/test_lockstep_gpu.py).

``LockstepGroup`` owns the C object; ``fit_lockstep`` is ``NeuralNetClassifier.partial_fit`` for K estimators at once
(the per-epoch callbacks are the same ``_FitRun`` code); ``fit_and_score_group`` is what ``ShardedGridSearchCV(lockstep=k)``
calls per work unit.
"""
import ctypes as C
import time

import numpy as np
import torch

from . import ops
from ._lib import check, load, ptr, stream_ptr

TRAIN, VALID, TEST = 0, 1, 2


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[ptr(t) for t in tensors])


class LockstepGroup:
    """The fits' engines -- all TransformerEngines or all RnnEngines, same configuration up to the dropout rate -- stepping
    together."""

    def __init__(self, engines):
        cfg = engines[0].cfg
        self.engines, self.K, self.device = list(engines), len(engines), engines[0].device
        self.kind = engines[0].prefix                    # "tf" / "rnn": the C family
        assert all(type(e) is type(engines[0]) for e in engines), "lockstep: one engine type per group"
        nbytes = int(self._fn("workspace_bytes")(C.byref(cfg), self.K))
        if nbytes < 0:
            raise RuntimeError("lockstep: bad configuration")
        self._alloc_stream = self._last_stream = torch.cuda.current_stream(self.device)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        handles = (C.c_void_p * self.K)(*[e.handle for e in self.engines])
        out = C.c_void_p()
        check(self._fn("create")(handles, self.K, ptr(self.workspace), nbytes, self._sp(), C.byref(out)), f"{self.kind}_lockstep_create")
        self.handle = out
        check(self._fn("set_destroy_sync")(out, 0), "lockstep_set_destroy_sync")   # torch-allocated tables: see _engine.py
        self.data, self.logp, self.loss, self.rows, self.n_visit, self._orders = {}, {}, {}, {}, {}, {}
        self.cap = {}                                    # rows the slot's output buffers hold (set_data: visit_rows)

    def _fn(self, name):                                 # a method, not a closure over self: no reference cycle
        return getattr(load(), f"slnlp_{self.kind}_lockstep_{name}")

    def _sp(self):
        st = self._last_stream = torch.cuda.current_stream(self.device)
        return st.cuda_stream

    def close(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            ls, al = getattr(self, "_last_stream", None), getattr(self, "_alloc_stream", None)
            if ls is not None and al is not None and ls != al:
                ls.synchronize()                         # the tables go back to another stream's pool (_engine.PlanEngine.__del__)
            self._fn("destroy")(h)

    __del__ = close

    def set_data(self, slot, Xs, ys, batch, lengths=None, visit_rows=None):
        """Per-fit datasets of one slot (device int64 [rows, S] / [rows], the same number of rows for every fit; RNN fits also
        pass the sequence lengths [rows]).  Allocates the slot's output buffers: ``logp[slot][f]`` [rows, Vt] and
        ``loss[slot][f]`` [ceil(rows / batch)] -- for ``max(rows, visit_rows)`` rows when a pass will visit more rows than the
        data has (class-balanced epochs: ``set_order`` with a table per fit)."""
        rows = int(Xs[0].shape[0])
        assert len(Xs) == len(ys) == self.K and all(x.shape[0] == rows and x.is_contiguous() for x in Xs)
        Vt = self.engines[0].cfg.Vt
        cap = max(rows, int(visit_rows or 0))
        nb = (cap + batch - 1) // batch
        self.logp[slot] = [torch.empty(cap, Vt, dtype=torch.float32, device=self.device) for _ in range(self.K)]
        self.loss[slot] = [torch.zeros(nb, dtype=torch.float32, device=self.device) for _ in range(self.K)]
        self.rows[slot], self.cap[slot] = rows, cap
        self.n_visit.pop(slot, None)                     # the C side drops the slot's order with its old data
        self._orders.pop(slot, None)
        if self.kind == "rnn":
            assert lengths is not None and len(lengths) == self.K, "lockstep: RNN fits need the sequence lengths"
            lengths = [l.contiguous() for l in lengths]
            self.data[slot] = (list(Xs), list(ys), lengths)   # keep the tensors alive: the C side holds raw pointers
            check(self._fn("set_data")(self.handle, slot, _ptr_array(Xs), _ptr_array(ys), _ptr_array(lengths), rows,
                                       _ptr_array(self.logp[slot]), _ptr_array(self.loss[slot]), self._sp()), "rnn_lockstep_set_data")
        else:
            self.data[slot] = (list(Xs), list(ys))
            check(self._fn("set_data")(self.handle, slot, _ptr_array(Xs), _ptr_array(ys), rows,
                                       _ptr_array(self.logp[slot]), _ptr_array(self.loss[slot]), self._sp()), "tf_lockstep_set_data")

    def set_adam(self, exp_avg_sq, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """Train with the fused clip + Adam update from now on; ``exp_avg_sq``: one arena-shaped buffer per fit."""
        assert len(exp_avg_sq) == self.K
        self._v2 = list(exp_avg_sq)                      # keep the tensors alive: the C side holds raw pointers
        check(self._fn("set_adam")(self.handle, _ptr_array(self._v2), betas[0], betas[1], eps, weight_decay), f"{self.kind}_lockstep_set_adam")

    def set_averaging(self, avgs=None, kind="swa", decay=0.0):
        """Weight averaging riding the group's train steps: ``avgs`` holds, per fit, ``(avg, count)`` -- the arena-shaped running
        average and its [1] float count (``ArenaModule.averaged_arena``) -- or None for a fit that is not averaging yet; one
        ``(kind, decay)`` for the group.  One launch over the K arenas per step.  ``avgs`` None (or all None): off.  A change makes
        the group record its programs again."""
        from ._lib import AVERAGE_KINDS
        given = [a for a in (avgs or []) if a is not None]
        if not given:
            self._avgs = None
            check(self._fn("set_averaging")(self.handle, None, None, 0, 0.0), f"{self.kind}_lockstep_set_averaging")
            return
        assert len(avgs) == self.K and all(a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() and a.numel() == e.arena_floats
                                           for (a, _), e in zip([x for x in avgs if x is not None],
                                                                [e for x, e in zip(avgs, self.engines) if x is not None])), \
            "lockstep: one (arena-shaped float32 device tensor, count) pair or None per fit"
        self._avgs = list(avgs)                          # keep the tensors alive: the step's launches write them
        a = (C.c_void_p * self.K)(*[None if x is None else ptr(x[0]) for x in avgs])
        c = (C.c_void_p * self.K)(*[None if x is None else ptr(x[1]) for x in avgs])
        check(self._fn("set_averaging")(self.handle, a, c, AVERAGE_KINDS[kind], float(decay)), f"{self.kind}_lockstep_set_averaging")

    def set_lr_tables(self, tables, n_steps=None):
        """Per-fit learning rates by train-batch index: a list with, per fit, a contiguous float32 device tensor [n_steps] or None
        (that fit keeps the rate its engine's ``set_lr`` gave it); None (or no tensor at all) clears the setting.  From then on every
        TRAIN step first stores ``tables[f][step_index]`` into fit f's learning rate, inside the launch that stages the batch.
        A fit whose engine has param groups (``set_param_groups``, G groups) gives [n_steps, G]: row ``step_index`` goes to its G
        group rates; ``n_steps`` (default: the first tensor's length) is then the one number the tensors share."""
        given = [t for t in (tables or []) if t is not None]
        if not given:
            self._lr_tables = None
            check(self._fn("set_lr_table")(self.handle, None, 0, self._sp()), f"{self.kind}_lockstep_set_lr_table")
            return
        n = int(given[0].shape[0]) if n_steps is None else int(n_steps)
        width = [1 if getattr(e, "_group_lr", None) is None else int(e._group_lr.numel()) for e in self.engines]
        assert len(tables) == self.K and all(t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n * w and
                                                           t.device == given[0].device)
                                             for t, w in zip(tables, width)), \
            "lockstep: one float32 device tensor [n_steps] ([n_steps, groups] with param groups) or None per fit"
        self._lr_tables = list(tables)                   # keep the tensors alive: the gather launch reads them
        arr = (C.c_void_p * self.K)(*[None if t is None else ptr(t) for t in tables])
        check(self._fn("set_lr_table")(self.handle, arr, n, self._sp()), f"{self.kind}_lockstep_set_lr_table")

    def set_order(self, slot, orders, n_visit=None):
        """Per-fit visit order of a slot (a shuffled epoch): a list with, per fit, a contiguous int64 device tensor [n_visit] of row
        indices into that fit's dataset or None (that fit stays in dataset order); ``orders`` None clears the setting.  ``n_visit``
        (default: the tensors' length) is the number of rows a pass visits, one number for the group -- with every entry None it
        only shortens the pass (drop_last).  From then on ``step`` / ``epoch`` stage row ``orders[f][row0 + i]`` for visit
        ``row0 + i``; log-probs and losses land at visit position, and ``results`` covers ``n_visit`` rows.  The indices are the
        caller's contract: check the host array (``slnlp.sampler.check_order``) before uploading it."""
        if orders is None:
            self.n_visit.pop(slot, None)
            self._orders.pop(slot, None)
            check(self._fn("set_order")(self.handle, slot, None, 0, self._sp()), f"{self.kind}_lockstep_set_order")
            return
        given = [t for t in orders if t is not None]
        n = int(given[0].numel()) if n_visit is None else int(n_visit)
        assert len(orders) == self.K and all(t.dtype == torch.int64 and t.is_contiguous() and t.numel() == n and t.device == self.device
                                             for t in given), "lockstep: one int64 device tensor [n_visit] (or None) per fit"
        # a pass longer than the data (tables that name rows more than once) writes n rows of log-probs: set_data(visit_rows=)
        # (only when every fit has a table: otherwise the library itself refuses a pass longer than the data)
        if len(given) == self.K and slot in self.cap and n > self.cap[slot]:
            raise ValueError(f"lockstep: n_visit {n} beyond the {self.cap[slot]} rows of the slot's output buffers")
        arr = (C.c_void_p * self.K)(*[None if t is None else ptr(t) for t in orders])
        check(self._fn("set_order")(self.handle, slot, arr, n, self._sp()), f"{self.kind}_lockstep_set_order")
        self._orders[slot] = list(orders)                # keep the tensors alive: the gather launch reads them
        self.n_visit[slot] = n

    def _sync_versions(self):
        for e in self.engines:                           # Transformer: weight planes follow outside writes to the fp32 arena
            if hasattr(e, "sync_params_version"):
                e.sync_params_version()

    def step(self, slot, row0, B, step_index, train, momentum=0.9, max_norm=0.5):
        self._sync_versions()
        check(self._fn("step")(self.handle, slot, row0, B, step_index, int(train), momentum, max_norm, self._sp()),
              f"{self.kind}_lockstep_step")

    def epoch(self, slot, batch, train, momentum=0.9, max_norm=0.5):
        """One pass over the slot in dataset order (or the slot's order tables: ``set_order``); no host synchronisation.
        Results: ``logp[slot]``, ``loss[slot]``."""
        self._sync_versions()
        check(self._fn("epoch")(self.handle, slot, batch, int(train), momentum, max_norm, self._sp()), f"{self.kind}_lockstep_epoch")

    def num_launches(self, slot, B, train):
        return int(self._fn("num_launches")(self.handle, slot, B, int(train)))

    def results(self, slot, f, batch):
        """What ``NeuralNetClassifier._run_epoch`` returns for fit ``f``: (batch-size weighted mean loss, log-probs [rows, Vt],
        [(batch loss, batch size)]) -- over the ``n_visit`` rows of a pass, in visit order, when the slot has an order.  Call
        after a synchronisation point."""
        rows = self.n_visit.get(slot, self.rows[slot])
        sizes = [min(batch, rows - r) for r in range(0, rows, batch)]
        per_batch, logp = self.loss[slot][f], self.logp[slot][f]
        if rows != self.cap[slot]:
            per_batch, logp = per_batch[:len(sizes)], logp[:rows]
        per_batch = per_batch.float().cpu()
        w = torch.tensor(sizes, dtype=torch.float32)
        mean = float((per_batch * w).sum() / w.sum())
        return mean, logp, list(zip(per_batch.tolist(), sizes))


LOCKSTEP_MODULES = ("Transformer", "EncoderDecoderLSTMAttn", "EncoderDecoderGRUAttn")


def lockstep_supported(net):
    """A fused update (SGD-momentum or Adam) + CrossEntropyLoss on one of the path's three modules: what the lockstep launch
    sequences implement."""
    return getattr(net, "_fused_kind", None) in ("sgd", "adam", "adamw") and type(net.module_).__name__ in LOCKSTEP_MODULES


def _adam_key(net):
    """What the fits of one group must share about their update: the kind and, for Adam / AdamW, the constants the group passes
    to every fit (betas, eps).  The weight decay (each plan's own once its kind is Adam / AdamW: slnlp_*_set_update), SGD's
    dampening / weight decay / nesterov, the criterion settings and the param groups (``optimizer__param_groups``: the table
    pointer and the rates' pointer) are each fit's own (they ride its argument packs)."""
    from .net import adam_args
    return (net._fused_kind,) + (adam_args(net)[:2] if net._fused_kind in ("adam", "adamw") else ())


def _avg_key(net):
    """What the fits of one group must share about weight averaging (``weight_averaging``): one (kind, decay, every) per group,
    or None for all.  ``start_epoch`` and ``predict`` are each fit's own: a fit whose epoch has not come rides the group's
    averaging launch with a null entry."""
    av = getattr(net, "_avg_opts", None)
    return None if av is None else (av["kind"], av["decay"], av["every"])


def _eval_pass(nets, data, bs):
    """One lockstep eval pass (the TEST slot) of ``nets`` over ``data`` -- per fit (X, lengths, y) on the device -- under the
    weights ``predict_proba`` evaluates with: the averaged ones stand in where ``weight_averaging`` predicts with them, and the
    live weights come back bit for bit.  Returns (group, the fits' log-probs: the group's own buffers); the caller closes the
    group.  No host wait."""
    S = data[0][0].shape[1]
    engines = [n.module_.engine(bs, S) for n in nets]
    for n in nets:
        n.module_.eval()
    group = LockstepGroup(engines)
    group.set_data(TEST, [d[0] for d in data], [d[2] for d in data], bs, [d[1] for d in data])
    swapped = [n for n in nets if n._predict_averaged()]
    for n in swapped:
        n.module_.swap_averaged()
    try:
        group.epoch(TEST, bs, False)
    finally:
        for n in swapped:
            n.module_.swap_averaged()
    return group, group.logp[TEST]


def _calibrate_lockstep(nets, runs, stream):
    """``NeuralNetClassifier._calibrate`` for the fits of a group whose ``calibration`` option is on: one lockstep eval pass over
    their valid splits, one ``fit_temperature`` / ``fit_bias_temperature`` call per fit on the group's stream (``fit_calibration``),
    then one sync and the downloads.  The fits whose
    ``conformal`` option is on then take their threshold on the same log-probs, at their temperature (``_conformalize_fit``)."""
    from .net import download_calibration, fit_calibration, stream_sync
    on = lambda n, key: getattr(n, key, None) is not None
    todo = [(n, r) for n, r in zip(nets, runs) if on(n, "_cal_opts") or on(n, "_conf_opts")]
    if not todo:
        return
    if any(r.va is None for n, r in todo if on(n, "_cal_opts")):
        raise ValueError("calibration: the fit has no valid split to fit the temperature on (train_split)")
    if any(r.va is None for _, r in todo):
        raise ValueError("conformal: the fit has no valid split to take the threshold on (train_split)")
    group, logps = _eval_pass([n for n, _ in todo], [(r.Xva, r.Lva, r.yva) for _, r in todo], todo[0][1].bs)
    fitted = [fit_calibration(n._cal_opts, lp, r.yva) if on(n, "_cal_opts") else None for lp, (n, r) in zip(logps, todo)]
    stream_sync(stream)
    for (n, _), got in zip(todo, fitted):
        if got is not None:
            n._set_calibration(*download_calibration(n._cal_opts, got))
    # the conformal option, as NeuralNetClassifier._conformalize_fit: after the temperature, on the same log-probs
    conf = [(n, r, n._conformal_calibrate(lp, r.yva, n._conf_opts, True)) for lp, (n, r) in zip(logps, todo) if on(n, "_conf_opts")]
    stream_sync(stream)
    group.close()
    for n, r, (state, use) in conf:
        n._set_conformal(n._conf_opts, state, use, labels=r.va.y, where="the valid data")


def fit_lockstep(nets, datasets):
    """``net.partial_fit(ds)`` for every (net, ds) pair, all fits advancing together.  The nets must be initialised,
    of one shape (lr and dropout rate may differ) and their datasets of one size; fits that stop early (EarlyStopping)
    leave the group, the others go on.  Fits whose ``calibration`` / ``conformal`` option is on are calibrated / conformalised after
    the last one has ended."""
    nets[0]._gate.enter(False)                          # fused fits share the device (slnlp.net: _DeviceGate)
    try:
        return _fit_lockstep_gated(nets, datasets)
    finally:
        nets[0]._gate.leave(False)


# tools/bench_grid_long.py sets EPOCH_LOG = [] to get one record per lockstep unit: how many fits were still training in each
# epoch and how long the epoch took (fits that stop early -- EarlyStopping, helper.py:240-250 -- leave the group, which is
# rebuilt from the fits that are left: `regroups`)
EPOCH_LOG = None


def _fit_lockstep_gated(nets, datasets):
    from .net import _FitRun, stream_sync
    import time
    K = len(nets)
    log = {"fits": K, "epochs": [], "regroups": 0} if EPOCH_LOG is not None else None
    stream = nets[0]._stream
    assert all(n._stream is stream for n in nets), "lockstep: the fits of a group share the device's stream"
    nets[0]._enter_stream()                             # the stream waits for whatever this thread queued elsewhere so far
    for n in nets:
        if getattr(n, "_cal_opts", None) is not None:
            n._set_calibration(None)                    # as partial_fit: an earlier fit's temperature does not describe these weights
        if getattr(n, "_conf_opts", None) is not None:
            n._set_conformal(None)
    with torch.cuda.stream(stream):
        runs = [_FitRun(n, d) for n, d in zip(nets, datasets)]
    r0 = runs[0]
    assert all(lockstep_supported(n) for n in nets), "lockstep: fused SGD / Adam / AdamW + CrossEntropyLoss on the model.* modules only"
    assert len({type(n.module_) for n in nets}) == 1, "lockstep: one module class per group"
    assert len({_adam_key(n) for n in nets}) == 1, "lockstep: one optimizer (and one set of Adam constants) per group"
    assert len({_avg_key(n) for n in nets}) == 1, "lockstep: one weight_averaging (kind, decay, every) per group"
    adam = _adam_key(nets[0]) if nets[0]._fused_kind in ("adam", "adamw") else None
    avg = _avg_key(nets[0])
    assert all((r.bs, r.momentum, r.max_norm, len(r.tr), r.n_visit, (len(r.va) if r.va is not None else 0)) ==
               (r0.bs, r0.momentum, r0.max_norm, len(r0.tr), r0.n_visit, (len(r0.va) if r0.va is not None else 0)) for r in runs), \
        "lockstep: the fits of a group share batch size, momentum, clipping, split sizes and drop_last"
    S = r0.Xtr.shape[1]
    with torch.cuda.stream(stream):
        engines = [n.module_.engine(r0.bs, S) for n in nets]
    active, group = [i for i in range(K) if not runs[i].done], None
    members = None
    with torch.cuda.stream(stream):
        while active:
            if members != active:                       # a fit left (or first epoch): regroup the ones still training
                if group is not None:
                    stream_sync(stream)
                    group.close()
                    if log is not None:
                        log["regroups"] += 1
                group = LockstepGroup([engines[i] for i in active])
                if adam is not None:
                    # weight_decay: each plan's own (NeuralNetClassifier.initialize set its update kind), not the group's
                    group.set_adam([nets[i].module_.adam_second_moment() for i in active], adam[1], adam[2], 0.0)
                group.set_data(TRAIN, [runs[i].Xtr for i in active], [runs[i].ytr for i in active], r0.bs,
                               [runs[i].Ltr for i in active], visit_rows=r0.n_visit)
                if r0.va is not None:
                    group.set_data(VALID, [runs[i].Xva for i in active], [runs[i].yva for i in active], r0.bs,
                                   [runs[i].Lva for i in active])
                members = list(active)
            # every fit's rates for this epoch, before anything is queued (a scheduler stepped past its end raises here)
            tables = [runs[i].lr_table() for i in active]
            orders = [runs[i].order() for i in active]  # shuffled fits: the epoch's visit order (host), drawn before anything is queued
            for i in active:
                engines[i].set_lr(nets[i].lr_)
                if nets[i]._groups is not None:
                    nets[i].module_.set_group_lrs(nets[i]._lrs)     # what a grouped fit's update reads instead
                nets[i].module_.train()
                runs[i].begin_epoch()
            pb = [j for j, (i, t) in enumerate(zip(active, tables)) if t is not None and runs[i].schedule.per_batch]
            if pb:
                # the epoch runs without coming back to the host: per-batch rates go to the device as one [fits, batches] tensor
                # (a host-to-device copy on the fit's stream, alive in the group until the next epoch replaces it), and each
                # step's gather launch hands every such fit its row's next entry; the other fits keep the rate set above
                # (a fit with param groups has G rates per step: its row is [batches, G], flattened)
                flat = [[v for row in tables[j] for v in (row if isinstance(row, list) else [row])] for j in pb]
                dev_tab = torch.tensor([v for f in flat for v in f], dtype=torch.float32).to(group.device)
                per_fit, at = [None] * len(active), 0
                for f, j in zip(flat, pb):
                    per_fit[j] = dev_tab[at:at + len(f)]
                    at += len(f)
                    if nets[active[j]]._groups is not None:
                        nets[active[j]].module_.forget_group_lrs()      # the device writes them from here on
                group.set_lr_tables(per_fit, n_steps=len(tables[pb[0]]))
            sh = [j for j, o in enumerate(orders) if o is not None]
            bal = [j for j, i in enumerate(active) if runs[i].balance is not None]
            if sh or bal or r0.n_visit != len(r0.tr):
                # the orders go to the device the same way: ONE [fits, 2, n_visit] tensor per epoch -- each shuffled fit's order and
                # its labels in visit order (what train scoring pairs the log-probs with) -- and every step's gather launch stages
                # the rows its fit's table names; unshuffled fits of the group keep dataset order (no table), and with drop_last
                # the group only visits the full batches.  A new group (after a regroup) gets its tables here like the first.
                per_fit = [None] * len(active)
                if sh:
                    dev_ord = torch.from_numpy(np.stack([runs[active[j]].visit_table() for j in sh])).to(group.device)
                    for r, j in enumerate(sh):
                        per_fit[j] = dev_ord[r, 0]
                        runs[active[j]].set_visit(dev_ord[r, 0], dev_ord[r, 1])
                for j in bal:                           # balanced fits: order() drew the table on the device, nothing to upload
                    per_fit[j] = runs[active[j]].order_dev
                group.set_order(TRAIN, per_fit, r0.n_visit)
            averaging = [nets[i]._averaging_epoch() for i in active]   # per fit: has its start_epoch come?
            if avg is not None and avg[2] == "batch":
                # the accumulator rides every train step, one launch over the group's arenas; a fit that is not averaging yet has a
                # null entry (a call that changes nothing costs nothing: the group re-records only when an entry moved)
                group.set_averaging([nets[i].module_.averaged_arena() if on else None for i, on in zip(active, averaging)], avg[0], avg[1])
            t_epoch = time.perf_counter()
            group.epoch(TRAIN, r0.bs, True, r0.momentum, r0.max_norm)
            if avg is not None and avg[2] == "epoch":
                for i, on in zip(active, averaging):    # behind the epoch's last step, in front of the valid pass; no host wait
                    if on:
                        nets[i].module_.average_now(avg[0], avg[1])
            if r0.va is not None:
                group.epoch(VALID, r0.bs, False, r0.momentum, r0.max_norm)
            stream_sync(stream)                         # one host sync per epoch for all K fits
            nxt = []
            for j, i in enumerate(active):
                tr = group.results(TRAIN, j, r0.bs)
                va = group.results(VALID, j, r0.bs) if r0.va is not None else None
                if not runs[i].end_epoch(tr, va):
                    nxt.append(i)
            if log is not None:
                log["epochs"].append([len(active), time.perf_counter() - t_epoch])
            active = nxt
    stream_sync(stream)
    if group is not None:
        group.close()
    with torch.cuda.stream(stream):
        _calibrate_lockstep(nets, runs, stream)
    if log is not None:
        log["epochs_run"] = [len(n.history) for n in nets]
        EPOCH_LOG.append(log)
    return nets


def predict_proba_lockstep(nets, datasets):
    """``net.predict_proba(ds)`` for every pair through one launch sequence (eval-mode forward, softmax of the log-probs as
    skorch's predict_nonlinearity='auto' does)."""
    from .net import stream_sync
    bs = int(nets[0].batch_size)
    nets[0]._gate.enter(False)
    try:
        return _predict_proba_lockstep_gated(nets, datasets, bs, stream_sync)
    finally:
        nets[0]._gate.leave(False)


def _predict_proba_lockstep_gated(nets, datasets, bs, stream_sync):
    nets[0]._enter_stream()
    with torch.cuda.stream(nets[0]._stream):
        group, logps = _eval_pass(nets, [n._device_data(d) for n, d in zip(nets, datasets)], bs)
        out = [lp.clone() for lp in logps]
        for n, o in zip(nets, out):
            n._calibrated_values(o, n._uses_temperature(True))   # a calibrated fit's log-probs become the calibrated ones, in place
        stream_sync(nets[0]._stream)
        # softmax on the host copies (torch's CPU op, as in NeuralNetClassifier.predict_proba: no torch arithmetic kernel runs
        # beside other fits on the GPU)
        out = [(torch.softmax(o.cpu(), dim=-1) if n.predict_nonlinearity == "auto" else o.cpu()).numpy() for n, o in zip(nets, out)]
        group.close()
    return out


def fit_and_score_group(estimator_factory, params_list, trains, tests, scoring="neg_log_loss", seeds=None):
    """``grid.default_fit_and_score`` for the tasks of one work unit: fresh estimators (seeded one after another, like the
    one-at-a-time path), one lockstep fit, one lockstep scoring pass over the test folds.  Falls back to one fit at a time for
    anything the lockstep sequence does not implement (other modules / optimizers) -- same results, just not merged."""
    from .grid import default_fit_and_score
    from .net import INIT_LOCK, ScoringWrapper, _CachedPredictor
    seeds = seeds or [None] * len(params_list)
    nets = []
    for params, seed in zip(params_list, seeds):
        net = estimator_factory().set_params(**params)
        if "checkpoint_dir" in net.get_params():
            net.set_params(checkpoint_dir=None)
        with INIT_LOCK:
            if seed is not None:
                torch.manual_seed(seed)
            net.initialize()
        nets.append(net)
    if not all(lockstep_supported(n) for n in nets) or len({type(n.module_) for n in nets}) != 1 or len({_adam_key(n) for n in nets}) != 1 or \
            len({_avg_key(n) for n in nets}) != 1 or len({len(t) for t in trains}) != 1 or len({len(t) for t in tests}) != 1 or \
            (any(n._iterator_train_balance() for n in nets) and len({n._epoch_rows(t) for n, t in zip(nets, trains)}) != 1):
        # (the last one: a balanced epoch's length follows the fold's labels, and a group shares its batch count)
        del nets
        # concurrent=True: no hipGraph capture -- other host threads may be launching on the device's shared stream
        return [default_fit_and_score(estimator_factory, p, tr, te, scoring, seed=s, concurrent=True)
                for p, tr, te, s in zip(params_list, trains, tests, seeds)]
    fit_lockstep(nets, trains)
    probas = predict_proba_lockstep(nets, tests)
    scores = []
    for net, train, test, proba in zip(nets, trains, tests, probas):
        wr = ScoringWrapper(scoring, train.labels() if ScoringWrapper.needs_labels(scoring) else None)
        scores.append(float(wr(_CachedPredictor(proba, net.classes_), None, test.y)))
    return scores
