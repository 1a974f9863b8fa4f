"""GPU: learning-rate schedules on the fused step -- per-fit device tables in a lockstep group against solo steps with
``set_lr``, the estimator against its torch-stepped path, graph replay, lockstep against solo fits, resume and the grid.

The data is the small case of tests/test_loss_optim_options_gpu.py: 80 rows of length 12, batch 20 -> four train batches per
epoch, the last one short.  ``OneCycleLR`` always gets ``total_steps`` = the train batches the fit runs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(module__embedding_size=32, module__num_heads=4, module__num_layers=2, module__hidden_size=64)
RNN_CFG = dict(module__embedding_size=24, module__hidden_size=32, module__num_layers=2)
MODULES = {"tf": ("model.Transformer", CFG), "lstm": ("model.EncoderDecoderLSTMAttn", RNN_CFG),
           "gru": ("model.EncoderDecoderGRUAttn", RNN_CFG)}
ADAMW = dict(optimizer="torch.optim.AdamW", optimizer__weight_decay=1e-2, lr=3e-3)
BS, NB = 20, 4


def dataset(n=80):
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(n, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


def make_net(ds, module="tf", **kw):
    from slnlp.net import NeuralNetClassifier
    mod, cfg = MODULES[module]
    args = dict(module=mod, module__dropout=0.0, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y,
                module__batch_first=True, **cfg, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1,
                optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05, max_epochs=3, batch_size=BS, device="cuda",
                gradient_clipping={"gradient_clip_value": 0.5})
    if kw.get("optimizer") == "torch.optim.AdamW":
        args.pop("optimizer__momentum")
    args.update(kw)
    return NeuralNetClassifier(**args)


def torch_rates(policy, n, lr, **kw):
    """The oracle: the rate in force before each of ``n`` optimizer steps of a real torch optimizer."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sch = getattr(torch.optim.lr_scheduler, policy)(opt, **kw)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    return out


def strip(history):
    return [{k: v for k, v in row.items() if k != "dur"} for row in history]


def same_weights(a, b):
    sa, sb = a.module_.state_dict(), b.module_.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------------------------------------------------ C ABI ----
def _engines(ds, module, seeds):
    """Fresh modules (own weights per seed) and the train part of the estimator's split on the device."""
    nets = []
    for s in seeds:
        torch.manual_seed(s)
        nets.append(make_net(ds, module).initialize())
    idx_tr, _ = nets[0]._train_split(ds)
    tr = ds[idx_tr]
    assert len(tr) == 64                                   # 20 + 20 + 20 + 4
    return nets, [n.module_.engine(BS, ds.ids.shape[1]) for n in nets], nets[0]._device_data(tr)


@pytest.mark.parametrize("module", list(MODULES))
def test_lockstep_lr_tables_equal_solo_steps_with_set_lr(module):
    from slnlp.lockstep import LockstepGroup, TRAIN, VALID
    ds = dataset()
    K = 3
    tables = [torch_rates("ExponentialLR", NB, 0.05, gamma=0.5), torch_rates("CosineAnnealingLR", NB, 0.03, T_max=4),
              torch_rates("OneCycleLR", NB, 0.01, max_lr=0.08, total_steps=NB, cycle_momentum=False)]
    assert len({tuple(t) for t in tables}) == K
    keep, solo, (X, L, y) = _engines(ds, module, (31, 32, 33))
    keep2, lock, _ = _engines(ds, module, (31, 32, 33))
    keep3, plain, _ = _engines(ds, module, (31, 32, 33))
    torch.cuda.synchronize()
    st = keep[0]._stream                                   # the stream the modules' buffers live on
    assert all(n._stream is st for n in keep + keep2 + keep3)
    with torch.cuda.stream(st):
        # ---- solo: one plan at a time, set_lr before every train step
        want = []
        for f, e in enumerate(solo):
            losses, logps = [], []
            for i, r in enumerate(range(0, X.shape[0], BS)):
                e.set_lr(tables[f][i])
                lp = e.step(X[r:r + BS], y[r:r + BS], L[r:r + BS], 0.9, 0.5, graph=False)
                losses.append(e.scalars[0].clone()); logps.append(lp.clone())
            want.append((torch.stack(losses), torch.cat(logps), e.params.clone(), e.momentum.clone()))
        # ---- the same three plans in a group, the rates delivered on the device
        for e in lock:
            e.set_lr(0.777)                                # every train step must overwrite this
        grp = LockstepGroup(lock)
        data = ([X] * K, [y] * K, BS, [L] * K)
        grp.set_data(TRAIN, *data)
        grp.set_data(VALID, *data)
        dev = [torch.tensor(t, dtype=torch.float32, device="cuda") for t in tables]
        grp.set_lr_tables(dev)
        grp.epoch(TRAIN, BS, True, 0.9, 0.5)
        st.synchronize()
        for f, e in enumerate(lock):
            losses, logps, params, mom = want[f]
            assert torch.equal(grp.loss[TRAIN][f], losses) and torch.equal(grp.logp[TRAIN][f], logps), f
            assert torch.equal(e.params, params) and torch.equal(e.momentum, mom), f
            assert float(e.lr) == float(dev[f][NB - 1])
        n_full, n_tail = grp.num_launches(TRAIN, BS, True), grp.num_launches(TRAIN, 4, True)
        assert n_full > 0 and n_tail > 0
        # ---- eval steps never touch the rate
        grp.epoch(VALID, BS, False)
        st.synchronize()
        assert [float(e.lr) for e in lock] == [float(d[NB - 1]) for d in dev]
        # ---- a batch index past the tables is an argument error, and nothing runs
        before = [e.params.clone() for e in lock]
        with pytest.raises(RuntimeError, match="learning-rate"):
            grp.step(TRAIN, 0, BS, NB, True, 0.9, 0.5)
        st.synchronize()
        assert all(torch.equal(e.params, b) for e, b in zip(lock, before))
        # ---- a NULL entry leaves that fit's rate at its set_lr value; changing the tables drops no program
        lock[1].set_lr(0.125)
        grp.set_lr_tables([dev[0], None, dev[2]])
        assert grp.num_launches(TRAIN, BS, True) == n_full and grp.num_launches(TRAIN, 4, True) == n_tail
        grp.step(TRAIN, 0, BS, 1, True, 0.9, 0.5)
        st.synchronize()
        assert [float(e.lr) for e in lock] == [float(dev[0][1]), 0.125, float(dev[2][1])]
        # ---- cleared: no fit's rate is touched any more, still the same programs
        for e in lock:
            e.set_lr(0.25)
        grp.set_lr_tables(None)
        assert grp.num_launches(TRAIN, BS, True) == n_full
        grp.step(TRAIN, 0, BS, 0, True, 0.9, 0.5)
        st.synchronize()
        assert [float(e.lr) for e in lock] == [0.25] * K
        # ---- the tables survive the workspace reclaim that follows a plan's settings change (programs re-recorded)
        grp.set_lr_tables(dev)
        lock[0].set_criterion(label_smoothing=0.1)
        grp.step(TRAIN, 0, BS, 2, True, 0.9, 0.5)
        st.synchronize()
        assert [float(e.lr) for e in lock] == [float(d[2]) for d in dev]
        assert grp.num_launches(TRAIN, BS, True) == n_full
        grp.close()
        # ---- a group that never had tables issues the same number of launches
        for e in plain:
            e.set_lr(0.01)
        grp2 = LockstepGroup(plain)
        grp2.set_data(TRAIN, *data)
        grp2.epoch(TRAIN, BS, True, 0.9, 0.5)
        st.synchronize()
        assert (grp2.num_launches(TRAIN, BS, True), grp2.num_launches(TRAIN, 4, True)) == (n_full, n_tail)
        assert [float(e.lr) for e in plain] == [float(torch.tensor(0.01, dtype=torch.float32))] * K
        grp2.close()


# --------------------------------------------------------------------------------------------------------- estimator ----
SCHEDULED = {
    "sgd_exponential_epoch": (dict(), {"policy": "ExponentialLR", "gamma": 0.7}),
    "adamw_onecycle_batch": (ADAMW, {"policy": "OneCycleLR", "step_every": "batch", "max_lr": 1e-2, "total_steps": 3 * NB,
                                     "cycle_momentum": False}),
}


@pytest.mark.parametrize("case", list(SCHEDULED))
@pytest.mark.parametrize("module", list(MODULES))
def test_fused_equals_torch_stepped_path_under_a_schedule(module, case):
    ds = dataset()
    opt, sched = SCHEDULED[case]
    nets = []
    for fused in (True, False):
        torch.manual_seed(11)
        net = make_net(ds, module, use_graph=False, lr_scheduler=dict(sched), **opt).initialize()
        assert net._fused
        if not fused:                                   # force the stock-optimizer path around the autograd bridge
            net._fused, net._fused_kind = False, None
            net.optimizer_ = net._opt_cls(net.module_.parameters(), lr=net.lr, **net._opt_kwargs)
        net.partial_fit(ds)
        nets.append(net)
    for key in ("train_loss", "valid_loss"):
        a, b = [h[key] for h in nets[0].history], [h[key] for h in nets[1].history]
        print(module, case, key, max(abs(x - y) / abs(y) for x, y in zip(a, b)))
        assert np.allclose(a, b, rtol=1e-4), (key, a, b)
    # both paths follow torch's own sequence, exactly
    kw = {k: v for k, v in sched.items() if k not in ("policy", "step_every")}
    per_batch = sched.get("step_every") == "batch"
    rates = torch_rates(sched["policy"], 3 * NB if per_batch else 3, nets[0].lr, **kw)
    for net in nets:
        events = [[b.get("event_lr") for b in h["batches"] if "train_loss" in b] for h in net.history]
        if per_batch:
            assert [v for e in events for v in e] == rates
            assert [h["lr"] for h in net.history[:-1]] == [rates[(e + 1) * NB] for e in range(2)]
            assert all("event_lr" not in b for h in net.history for b in h["batches"] if "valid_loss" in b)
        else:
            assert [h["lr"] for h in net.history] == rates
            assert all(v is None for e in events for v in e)
    assert nets[0].history[-1]["lr"] == nets[1].history[-1]["lr"]
    assert len(set(rates)) > 1


@pytest.mark.parametrize("module", list(MODULES))
def test_graph_replay_equals_eager_steps_under_a_per_batch_schedule(module):
    ds = dataset()
    sched = {"policy": "CosineAnnealingLR", "step_every": "batch", "T_max": 3 * NB, "eta_min": 1e-3}
    nets = []
    for graph in (True, False):
        torch.manual_seed(11)
        nets.append(make_net(ds, module, use_graph=graph, lr_scheduler=dict(sched)).fit(ds))
    assert strip(nets[0].history) == strip(nets[1].history) and same_weights(*nets)
    events = [b["event_lr"] for h in nets[0].history for b in h["batches"] if "train_loss" in b]
    assert events == torch_rates("CosineAnnealingLR", 3 * NB, 0.05, T_max=3 * NB, eta_min=1e-3)


# ---------------------------------------------------------------------------------------------------------- lockstep ----
def lock_schedules(epochs):
    return [{"policy": "StepLR", "step_size": 1, "gamma": 0.5},
            {"policy": "CosineAnnealingLR", "step_every": "batch", "T_max": epochs * NB},
            {"policy": "OneCycleLR", "step_every": "batch", "max_lr": 0.1, "total_steps": epochs * NB, "cycle_momentum": False},
            None]


@pytest.mark.parametrize("early_stop", [False, True], ids=["full", "one_fit_leaves_early"])
@pytest.mark.parametrize("module", list(MODULES))
def test_lockstep_fits_with_own_schedules_equal_solo_fits(module, early_stop):
    from slnlp.lockstep import fit_lockstep
    ds = dataset(100)
    parts = [ds[np.arange(i * 5, i * 5 + 80)] for i in range(4)]
    epochs = 5 if early_stop else 3
    # a threshold no epoch can meet after the first: that fit stops after `patience` more epochs, the others run on regrouped
    stops = [None, {"patience": 2, "threshold": 10.0, "threshold_mode": "abs"}, None, None] if early_stop else [None] * 4

    def build():
        nets = []
        for i, (sched, es) in enumerate(zip(lock_schedules(epochs), stops)):
            torch.manual_seed(40 + i)
            nets.append(make_net(ds, module, use_graph=False, scoring=["neg_log_loss"], max_epochs=epochs, lr_scheduler=sched,
                                 early_stopping=es).initialize())
        return nets
    solo = build()
    for n, d in zip(solo, parts):
        n.partial_fit(d)
    lock = build()
    fit_lockstep(lock, parts)
    for a, b in zip(solo, lock):
        assert a._fused and strip(a.history) == strip(b.history)
        assert same_weights(a, b)
    lens = [len(n.history) for n in lock]
    assert lens == ([epochs, 3, epochs, epochs] if early_stop else [epochs] * 4)
    # the schedules did run: torch's own sequences in the histories
    assert [h["lr"] for h in lock[0].history] == torch_rates("StepLR", epochs, 0.05, step_size=1, gamma=0.5)
    ev = lambda n: [b["event_lr"] for h in n.history for b in h["batches"] if "train_loss" in b]
    assert ev(lock[1]) == torch_rates("CosineAnnealingLR", lens[1] * NB, 0.05, T_max=epochs * NB)
    assert ev(lock[2]) == torch_rates("OneCycleLR", epochs * NB, 0.05, max_lr=0.1, total_steps=epochs * NB, cycle_momentum=False)
    assert [h["lr"] for h in lock[3].history] == [0.05] * epochs


# ------------------------------------------------------------------------------------------------------------ resume ----
@pytest.mark.parametrize("module", list(MODULES))
def test_resume_continues_a_per_batch_schedule(tmp_path, module):
    ds = dataset()
    kw = dict(use_graph=False, lr_scheduler={"policy": "CosineAnnealingLR", "step_every": "batch", "T_max": 16})
    torch.manual_seed(3)
    full = make_net(ds, module, max_epochs=4, **kw).fit(ds)
    torch.manual_seed(3)
    first = make_net(ds, module, max_epochs=2, **kw).fit(ds)
    first.save_params(str(tmp_path))
    rates = torch_rates("CosineAnnealingLR", 17, 0.05, T_max=16)
    group = torch.load(tmp_path / "optimizer.pt")["param_groups"][0]
    assert type(group["lr"]) is float and group["lr"] == rates[8]          # the current rate, as a double
    torch.manual_seed(99)
    resumed = make_net(ds, module, max_epochs=2, warm_start=True, **kw).initialize()
    resumed.load_params(str(tmp_path))
    resumed.partial_fit(ds)
    keys = ("epoch", "train_loss", "valid_loss", "lr", "batches")
    part = lambda h: [{k: row[k] for k in keys} for row in h]
    assert part(resumed.history[2:]) == part(full.history[2:])
    assert same_weights(resumed, full)
    assert [b["event_lr"] for h in resumed.history for b in h["batches"] if "train_loss" in b] == rates[:16]
    assert resumed.history[-1]["lr"] == rates[16]


# -------------------------------------------------------------------------------------------------------------- grid ----
def test_sharded_grid_lockstep_over_schedules(monkeypatch):
    from slnlp import grid as grid_mod
    from slnlp.grid import ShardedGridSearchCV
    ds = dataset(100)
    # cv=2 on 100 rows: 50 train rows per fold, 40 after the estimator's own split -> 2 train batches per epoch, 2 epochs
    grid = {"lr_scheduler": [{"policy": "StepLR", "step_size": 1, "gamma": 0.3},
                             {"policy": "OneCycleLR", "step_every": "batch", "max_lr": 0.2, "total_steps": 4, "cycle_momentum": False},
                             {"policy": "ExponentialLR", "step_every": "batch", "gamma": 0.6}]}
    factory = lambda: make_net(ds, max_epochs=2, use_graph=False, scoring=["neg_log_loss"])
    res = {1: ShardedGridSearchCV(factory, grid, cv=2, refit=False, device="cuda:0", lockstep=1).fit(ds)}
    one_at_a_time = []
    real = grid_mod.default_fit_and_score
    monkeypatch.setattr(grid_mod, "default_fit_and_score", lambda *a, **k: one_at_a_time.append(1) or real(*a, **k))
    res[4] = ShardedGridSearchCV(factory, grid, cv=2, refit=False, device="cuda:0", lockstep=4).fit(ds)
    assert not one_at_a_time                                          # every unit stepped in lockstep
    assert res[4].n_units_ < res[1].n_units_ == 6
    for key in ("mean_test_score", "split0_test_score", "split1_test_score"):
        assert np.array_equal(res[1].cv_results_[key], res[4].cv_results_[key]), key
    assert len(set(res[4].cv_results_["mean_test_score"])) == 3       # the schedules did differ
