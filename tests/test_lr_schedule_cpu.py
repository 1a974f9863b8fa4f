"""CPU: learning-rate schedules (slnlp/schedule.py) against torch's schedulers stepped directly, their translation from the
``lr_scheduler`` dict / the ``LRScheduler`` callback, their errors, and the grid's work units.

The oracle is always a torch scheduler on a real torch optimizer driven by the few lines of ``torch_sequence`` below, never
the module under test."""
import pytest
import torch

LR = 0.05
N_BATCHES, N_EPOCHS = 4, 3

POLICIES = {
    "StepLR": dict(step_size=3, gamma=0.5),
    "MultiStepLR": dict(milestones=[2, 5], gamma=0.1),
    "ExponentialLR": dict(gamma=0.9),
    "CosineAnnealingLR": dict(T_max=10, eta_min=1e-4),
    "CosineAnnealingWarmRestarts": dict(T_0=4, T_mult=2),
    "LinearLR": dict(start_factor=0.1, total_iters=5),
    "ConstantLR": dict(factor=0.5, total_iters=3),
    "PolynomialLR": dict(total_iters=6, power=2.0),
    "LambdaLR": dict(lr_lambda=lambda e: min(1.0, (e + 1) / 4)),
    "CyclicLR": dict(base_lr=0.01, max_lr=0.1, step_size_up=3, cycle_momentum=False),
    "OneCycleLR": dict(max_lr=0.1, total_steps=12, cycle_momentum=False),
}


def torch_sequence(policy, n, **kw):
    """The rate in force before each of ``n`` optimizer steps, the scheduler stepped after each."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=LR)
    sch = getattr(torch.optim.lr_scheduler, policy)(opt, **kw)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    return out


def fake_history(epochs, with_valid=True):
    """A skorch-layout history of ``epochs`` epochs of N_BATCHES train batches (and a valid batch, which counts for nothing)."""
    rows = []
    for e in range(epochs):
        batches = [{"train_loss": 1.0, "train_batch_size": 20} for _ in range(N_BATCHES)]
        if with_valid:
            batches.append({"valid_loss": 1.0, "valid_batch_size": 16})
        rows.append({"epoch": e + 1, "train_loss": 1.0, "batches": batches})
    return rows


@pytest.mark.parametrize("step_every", ["epoch", "batch"])
@pytest.mark.parametrize("policy", list(POLICIES))
def test_epoch_table_is_torch_own_sequence(policy, step_every):
    from slnlp.schedule import LRSchedule
    s = LRSchedule(policy, LR, step_every, **POLICIES[policy])
    got, at_end = [], []
    for _ in range(N_EPOCHS):
        table = s.epoch_table(N_BATCHES)
        assert len(table) == N_BATCHES and all(type(v) is float for v in table)
        got += table
        at_end.append(s.current)                            # what the epoch's history row reports as lr
        s.epoch_end()
    if step_every == "batch":
        want = torch_sequence(policy, N_EPOCHS * N_BATCHES + 1, **POLICIES[policy]) if policy != "OneCycleLR" else \
            torch_sequence(policy, N_EPOCHS * N_BATCHES, **POLICIES[policy]) + [None]
        assert got == want[:N_EPOCHS * N_BATCHES]
        # the rate after the epoch's last batch step: the one the next batch will use
        assert at_end[:-1] == [want[(e + 1) * N_BATCHES] for e in range(N_EPOCHS - 1)]
    else:
        per_epoch = torch_sequence(policy, N_EPOCHS, **POLICIES[policy])
        assert got == [v for v in per_epoch for _ in range(N_BATCHES)]
        assert at_end == per_epoch                          # read before the epoch-level step


@pytest.mark.parametrize("step_every", ["epoch", "batch"])
@pytest.mark.parametrize("policy", list(POLICIES))
def test_fast_forward_continues_the_uninterrupted_schedule(policy, step_every):
    from slnlp.schedule import LRSchedule
    total = N_EPOCHS * (N_BATCHES if step_every == "batch" else 1)
    want = torch_sequence(policy, total, **POLICIES[policy])
    for k in range(N_EPOCHS):
        s = LRSchedule(policy, LR, step_every, **POLICIES[policy]).fast_forward(fake_history(k))
        got = []
        for _ in range(N_EPOCHS - k):
            table = s.epoch_table(N_BATCHES)
            got += table if step_every == "batch" else table[:1]
            s.epoch_end()
        done = k * (N_BATCHES if step_every == "batch" else 1)
        assert got == want[done:], (policy, k)


def test_one_cycle_past_its_end_raises_torch_own_error():
    from slnlp.schedule import LRSchedule
    kw = POLICIES["OneCycleLR"]
    with pytest.raises(ValueError) as want:
        torch_sequence("OneCycleLR", 13, **kw)
    s = LRSchedule("OneCycleLR", LR, "batch", **kw)
    for _ in range(3):
        s.epoch_table(N_BATCHES)
    with pytest.raises(ValueError) as got:
        s.epoch_table(N_BATCHES)                            # a fourth 4-batch epoch of a 12-step cycle
    assert str(got.value) == str(want.value)
    with pytest.raises(ValueError) as got:                  # the same for a fit that resumes at the schedule's end
        LRSchedule("OneCycleLR", LR, "batch", **kw).fast_forward(fake_history(3)).epoch_table(N_BATCHES)
    assert str(got.value) == str(want.value)


def _callback(**kw):
    return type("LRScheduler", (), kw)()


def test_dict_and_callback_give_the_same_setting():
    from slnlp.net import NeuralNetClassifier
    from slnlp.schedule import LRSchedule
    kw = dict(T_max=10, eta_min=1e-4)
    a = NeuralNetClassifier(module="model.Transformer", lr=LR, lr_scheduler={"policy": "CosineAnnealingLR", "step_every": "batch", **kw})
    b = NeuralNetClassifier(module="model.Transformer", lr=LR,
                            callbacks=[("lr_scheduler", _callback(policy="CosineAnnealingLR", step_every="batch", monitor="valid_loss", kwargs=kw))])
    assert a.get_params()["lr_scheduler"] == b.get_params()["lr_scheduler"] == {"policy": "CosineAnnealingLR", "step_every": "batch", **kw}
    # step_every defaults to "epoch" in both forms; the class is accepted where the name is
    c = NeuralNetClassifier(module="model.Transformer", lr=LR,
                            callbacks=[_callback(policy=torch.optim.lr_scheduler.ExponentialLR, kwargs={"gamma": 0.9})])
    setting = c.get_params()["lr_scheduler"]
    assert setting["step_every"] == "epoch"
    for s in (LRSchedule.from_setting(setting, LR), LRSchedule.from_setting({"policy": "ExponentialLR", "gamma": 0.9}, LR)):
        assert not s.per_batch
        got = []
        for _ in range(3):
            got.append(s.epoch_table(2)[0])
            s.epoch_end()
        assert got == torch_sequence("ExponentialLR", 3, gamma=0.9)
    # the plateau's translation is what it was
    d = NeuralNetClassifier(module="model.Transformer", callbacks=[_callback(policy="ReduceLROnPlateau", monitor="valid_loss", step_every="epoch",
                                                                             kwargs={"factor": 0.2, "patience": 5})])
    assert d.get_params()["lr_scheduler"] == {"policy": "ReduceLROnPlateau", "factor": 0.2, "patience": 5}


@pytest.mark.parametrize("form", ["callback", "dict"])
def test_settings_the_loop_cannot_honour_raise_where_they_are_given(form):
    from slnlp.net import NeuralNetClassifier

    def give(policy, **kw):
        if form == "callback":
            return NeuralNetClassifier(module="model.Transformer", lr=LR, callbacks=[_callback(policy=policy, step_every="batch", kwargs=kw)])
        # the dict is checked by initialize(), ahead of anything that needs a GPU
        return NeuralNetClassifier(module="model.Transformer", lr=LR, lr_scheduler={"policy": policy, "step_every": "batch", **kw}).initialize()
    # momentum cycling (the default of both cyclic policies) is never silently dropped
    with pytest.raises(ValueError, match="cycle_momentum=False"):
        give("CyclicLR", base_lr=0.01, max_lr=0.1)
    with pytest.raises(ValueError, match="cycle_momentum=False"):
        give("OneCycleLR", max_lr=0.1, total_steps=12)
    with pytest.raises(ValueError, match="cycle_momentum=False"):
        give("OneCycleLR", max_lr=0.1, total_steps=12, cycle_momentum=True)
    with pytest.raises(ValueError, match="CosineAnnealingWarmRestarts"):
        give("WarmRestartLR", min_lr=1e-4)
    with pytest.raises(ValueError, match="CosineAnnealingWarmRestarts"):
        give(type("WarmRestartLR", (), {}))
    # a policy that cannot be constructed from its arguments: the message lists what is accepted
    for policy, kw in (("StepLR", {}), ("StepLR", {"no_such_argument": 1}), ("NoSuchLR", {}), ("OneCycleLR", {"max_lr": 0.1, "cycle_momentum": False})):
        with pytest.raises(ValueError, match="ReduceLROnPlateau") as e:
            give(policy, **kw)
        assert "step_every" in str(e.value) and "torch.optim.lr_scheduler" in str(e.value)


def test_bad_step_every_raises():
    from slnlp.net import NeuralNetClassifier
    with pytest.raises(ValueError, match="step_every"):
        NeuralNetClassifier(module="model.Transformer", callbacks=[_callback(policy="StepLR", step_every="step", kwargs={"step_size": 2})])


def test_candidates_that_differ_only_in_lr_scheduler_share_a_unit():
    import numpy as np
    from slnlp.grid import build_tasks, build_units
    grid = {"lr_scheduler": [{"policy": "StepLR", "step_size": 2}, {"policy": "CosineAnnealingLR", "step_every": "batch", "T_max": 8},
                             {"policy": "OneCycleLR", "step_every": "batch", "max_lr": 0.1, "total_steps": 8, "cycle_momentum": False}, None],
            "module__hidden_size": [32, 64]}
    y = np.arange(40) % 4
    cands, folds, tasks, order = build_tasks(grid, y, 2, seq_len=12)
    units = build_units(cands, folds, tasks, order, 4)
    assert len(cands) == 8 and len(tasks) == 16
    assert len(units) == 4 and all(len(u) == 4 for u in units)
    for u in units:                                         # a unit: one hidden size, several schedules (folds of one size mix)
        assert len({cands[tasks[t][0]]["module__hidden_size"] for t in u}) == 1
        assert len({repr(cands[tasks[t][0]]["lr_scheduler"]) for t in u}) >= 2


def test_cli_forwards_step_every_and_policy_arguments(tmp_path):
    """The YAML's lr_scheduler dict reaches the estimator whole, and a grid over lr_scheduler reaches the search."""
    from slnlp import cli
    from slnlp.data import synthetic_dataset
    from slnlp.net import NeuralNetClassifier
    cfg = tmp_path / "config.yaml"
    cfg.write_text("model: model.Transformer\nlr: 0.05\n"
                   "lr_scheduler: {policy: OneCycleLR, step_every: batch, max_lr: 0.1, total_steps: 12, cycle_momentum: false}\n"
                   "grid_args:\n  lr_scheduler:\n    - {policy: StepLR, step_size: 2}\n    - {policy: MultiStepLR, milestones: [2, 5], step_every: batch}\n")
    args = cli.load_config(str(cfg))
    want = {"policy": "OneCycleLR", "step_every": "batch", "max_lr": 0.1, "total_steps": 12, "cycle_momentum": False}
    ds = synthetic_dataset(20, seq_len=8, src_vocab=20, n_labels=3, seed=1, min_len=3)
    params = cli.build_net_params(args, ds, "cuda")
    assert params["lr_scheduler"] == want
    assert NeuralNetClassifier(**params).get_params()["lr_scheduler"] == want
    assert cli.build_param_grid(args["grid_args"])["lr_scheduler"] == [{"policy": "StepLR", "step_size": 2},
                                                                       {"policy": "MultiStepLR", "milestones": [2, 5], "step_every": "batch"}]
