"""CPU: which criterion / optimizer arguments run on the fused step (slnlp.net.fused_kind), and the grid's grouping of
candidates that differ only in per-fit criterion / update settings."""
import numpy as np
import pytest
import torch

from slnlp import grid
from slnlp.lockstep import _adam_key
from slnlp.net import criterion_options, fused_kind, update_options, optimizer_defaults


class _EngineModule:                 # stands in for a model.* class: fused_kind only asks whether it has `engine`
    engine = None


CE = torch.nn.CrossEntropyLoss
SGD = torch.optim.SGD


@pytest.mark.parametrize("crit, opt_cls, opt_kw, want", [
    (CE(ignore_index=1), SGD, {"momentum": 0.9}, "sgd"),
    (CE(ignore_index=1, label_smoothing=0.1), SGD, {"momentum": 0.9}, "sgd"),
    (CE(ignore_index=1, weight=torch.rand(6)), SGD, {"momentum": 0.9}, "sgd"),
    (CE(ignore_index=1, reduction="sum"), SGD, {"momentum": 0.9}, "sgd"),
    (CE(ignore_index=1, reduction="none"), SGD, {"momentum": 0.9}, None),
    (CE(ignore_index=1), SGD, {"momentum": 0.9, "nesterov": True}, "sgd"),
    (CE(ignore_index=1), SGD, {"momentum": 0.9, "dampening": 0.5}, "sgd"),
    (CE(ignore_index=1), SGD, {"momentum": 0.9, "weight_decay": 1e-4}, "sgd"),
    (CE(ignore_index=1), SGD, {"momentum": 0.9, "maximize": True}, None),
    (CE(ignore_index=1), torch.optim.Adam, {}, "adam"),
    (CE(ignore_index=1), torch.optim.Adam, {"amsgrad": True}, None),
    (CE(ignore_index=1), torch.optim.AdamW, {"weight_decay": 1e-3}, "adamw"),
    (CE(ignore_index=1), torch.optim.AdamW, {"amsgrad": True}, None),
    (CE(ignore_index=1), torch.optim.Adagrad, {}, None),
    (torch.nn.NLLLoss(ignore_index=1), SGD, {"momentum": 0.9}, None),
])
def test_fused_kind_table(crit, opt_cls, opt_kw, want):
    assert fused_kind(crit, opt_cls, opt_kw, _EngineModule) == want


def test_fused_kind_needs_a_library_module():
    assert fused_kind(CE(), SGD, {"momentum": 0.9}, torch.nn.Linear) is None


def test_fused_kind_raises_torchs_error_for_nesterov_with_dampening():
    with pytest.raises(ValueError) as ours:
        fused_kind(CE(ignore_index=1), SGD, {"momentum": 0.9, "nesterov": True, "dampening": 0.1}, _EngineModule)
    with pytest.raises(ValueError) as torchs:
        SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.01, momentum=0.9, nesterov=True, dampening=0.1)
    assert str(ours.value) == str(torchs.value)


def test_settings_pushed_to_the_engine():
    w = torch.rand(6)
    c = criterion_options(CE(ignore_index=1, weight=w, label_smoothing=0.2, reduction="sum"))
    assert torch.equal(c["weight"], w) and c["label_smoothing"] == pytest.approx(0.2) and c["reduction"] == "sum"
    assert criterion_options(CE(reduction="none")) is None
    d = optimizer_defaults(SGD, {"lr": 0.1, "momentum": 0.9, "nesterov": True, "weight_decay": 1e-4})
    assert update_options("sgd", d) == {"kind": "sgd", "dampening": 0.0, "weight_decay": 1e-4, "nesterov": True}
    # AdamW's torch default weight decay (1e-2) is what the fused step uses when the grid does not set one
    assert optimizer_defaults(torch.optim.AdamW, {})["weight_decay"] == pytest.approx(1e-2)
    assert update_options("adamw", optimizer_defaults(torch.optim.AdamW, {})) == {"kind": "adamw", "weight_decay": 1e-2}


def test_candidates_differing_in_per_fit_settings_share_a_lockstep_unit():
    y = np.repeat(np.arange(4), 10)
    param_grid = {"criterion__label_smoothing": [0.0, 0.1], "optimizer__weight_decay": [0.0, 1e-4],
                  "optimizer__dampening": [0.0, 0.5], "optimizer__nesterov": [False]}
    cands, folds, tasks, order = grid.build_tasks(param_grid, y, 2)
    assert len(cands) == 8 and len(tasks) == 16
    units = grid.build_units(cands, folds, tasks, order, lockstep=16)
    assert len(units) == 1 and sorted(units[0]) == list(range(16))
    # a shape key still splits
    cands, folds, tasks, order = grid.build_tasks({**param_grid, "module__num_layers": [1, 2]}, y, 2)
    assert len(grid.build_units(cands, folds, tasks, order, lockstep=32)) == 2


def _fused_net(opt_cls, **kw):
    from types import SimpleNamespace
    return SimpleNamespace(_fused_kind=fused_kind(CE(ignore_index=1), opt_cls, kw, _EngineModule),
                           _opt_defaults=optimizer_defaults(opt_cls, kw))


@pytest.mark.parametrize("opt_cls", [torch.optim.Adam, torch.optim.AdamW])
def test_adam_candidates_differing_in_weight_decay_share_a_lockstep_unit_and_group(opt_cls):
    """The Adam / AdamW weight decay is each fit's own (its plan's update settings), not a group constant: candidates that differ
    only in it share a unit, and the unit's fits have one group key (fit_and_score_group steps them in lockstep)."""
    y = np.repeat(np.arange(4), 10)
    cands, folds, tasks, order = grid.build_tasks({"optimizer__weight_decay": [0.0, 1e-4, 1e-2]}, y, 2)
    units = grid.build_units(cands, folds, tasks, order, lockstep=6)
    assert len(units) == 1 and len(units[0]) == 6
    opt_kw = [{k[len("optimizer__"):]: v for k, v in cands[tasks[t][0]].items()} for t in units[0]]
    assert len({kw["weight_decay"] for kw in opt_kw}) == 3
    assert len({_adam_key(_fused_net(opt_cls, **kw)) for kw in opt_kw}) == 1
    # what the group does share still splits: betas
    assert _adam_key(_fused_net(opt_cls, betas=(0.9, 0.99))) != _adam_key(_fused_net(opt_cls))
    assert update_options(_fused_net(opt_cls)._fused_kind, optimizer_defaults(opt_cls, {"weight_decay": 1e-4}))["weight_decay"] == 1e-4
