"""CPU: ``optimizer__param_groups`` on the host -- the group builder against skorch's rule (restated in the issue: pairs in
order, fnmatch over the names not yet taken, an empty match makes no group, the remainder is the last group), the fused
update's segment table, ``fused_kind`` with groups, per-group schedules against real torch schedulers on a real
multi-group optimizer, the checkpoint's position mapping, and the grid's work units."""
from fnmatch import fnmatch

import numpy as np
import pytest
import torch

from slnlp import grid, param_groups as pg
from slnlp.net import fused_kind, optimizer_kwargs

from test_loss_optim_options_cpu import CE, SGD, _EngineModule, test_fused_kind_table as _table_test
from test_lr_schedule_cpu import N_BATCHES, N_EPOCHS, POLICIES, fake_history

CFG = dict(embedding_size=32, num_heads=4, num_layers=2, hidden_size=64)
RNN_CFG = dict(embedding_size=24, hidden_size=32, num_layers=2)
MODULES = {"tf": ("Transformer", CFG), "lstm": ("EncoderDecoderLSTMAttn", RNN_CFG), "gru": ("EncoderDecoderGRUAttn", RNN_CFG)}

# the issue's pairs, plus a pattern that matches nothing and two overlapping ones ("*bias" is a subset of "*bias*"; "*norm*"
# takes the LayerNorm biases before either sees them)
PAIRS = [("*norm*", {"weight_decay": 0.0}), ("*bias", {"weight_decay": 0.0}), ("*no_such_parameter*", {"lr": 1.0}),
         ("*bias*", {"weight_decay": 0.0, "lr": 2e-3}), ("*embed*.weight", {"lr": 1e-4})]


def make_module(which):
    import model
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(80, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)
    name, cfg = MODULES[which]
    return getattr(model, name)(dropout=0.0, src_vocab=ds.vocab_X, tgt_vocab=ds.vocab_y, batch_first=True, **cfg)


def spec_groups(names, pairs):
    """The specification, written out independently of slnlp.param_groups: name -> index of the first matching pair."""
    first = {}
    for n in names:
        first[n] = next((i for i, (pat, _) in enumerate(pairs) if fnmatch(n, pat)), None)
    return first


@pytest.mark.parametrize("which", list(MODULES))
def test_builder_follows_the_specification(which):
    m = make_module(which)
    named = list(m.named_parameters())
    names = [n for n, _ in named]
    groups = pg.build(names, PAIRS)
    first = spec_groups(names, PAIRS)
    used = [i for i in range(len(PAIRS)) if i in set(first.values())]          # pairs that matched something, in order
    assert 2 not in used                                                          # the pattern that matches nothing: no group
    assert [g.pattern for g in groups] == [PAIRS[i][0] for i in used] + [None]    # remainder last
    for g, i in zip(groups, used + [None]):
        assert g.names == [n for n in names if first[n] == i]                     # membership, first match wins, named order
        assert g.settings == ({} if i is None else PAIRS[i][1])
    assert sorted(n for g in groups for n in g.names) == sorted(names)            # every parameter exactly once
    assert groups[0].pattern == ("*norm*" if which == "tf" else "*bias")          # which group is param_groups[0]
    if which == "tf":
        assert any(n.endswith("norm1.bias") for n in groups[0].names)             # overlap: the norm biases went to "*norm*"
        assert not any("norm" in n for g in groups[1:] for n in g.names)
    else:
        assert all("bias_" in n for n in groups[1].names) and groups[1].pattern == "*bias*"
    # torch builds exactly these groups from them
    opt = torch.optim.AdamW(pg.torch_groups(groups, named), lr=3e-3, weight_decay=1e-2)
    params = dict(named)
    assert len(opt.param_groups) == len(groups)
    for tg, g in zip(opt.param_groups, groups):
        assert len(tg["params"]) == len(g.names) and all(a is params[n] for a, n in zip(tg["params"], g.names))
        assert tg["lr"] == g.settings.get("lr", 3e-3) and tg["weight_decay"] == g.settings.get("weight_decay", 1e-2)
    assert pg.resolved(groups, opt.defaults, "lr") == [tg["lr"] for tg in opt.param_groups]
    assert pg.resolved(groups, opt.defaults, "weight_decay") == [tg["weight_decay"] for tg in opt.param_groups]


@pytest.mark.parametrize("which", list(MODULES))
def test_segment_table_covers_the_arena_once(which):
    m = make_module(which)
    names = [n for n, _ in m.named_parameters()]
    groups = pg.build(names, PAIRS)
    total = m._arena.numel()
    begin, group = pg.segments(groups, m._entries, total)
    assert len(begin) == len(group) and begin[0] == 0 and begin == sorted(set(begin)) and begin[-1] < total
    assert all(b % 4 == 0 for b in begin) and all(0 <= g < len(groups) for g in group)
    assert all(a != b for a, b in zip(group, group[1:]))                          # adjacent entries of one group are merged
    of = {n: gi for gi, g in enumerate(groups) for n in g.names}
    ends = begin[1:] + [total]
    owner = np.full(total, -1)
    for b, e, g in zip(begin, ends, group):
        assert (owner[b:e] == -1).all()
        owner[b:e] = g
    assert (owner >= 0).all()                                                     # the arena exactly once
    for name, shape, off in m._entries:
        n = int(np.prod(shape))
        assert (owner[off:off + n] == of[name]).all(), name                       # every float of a parameter in ITS group
    # one group: one segment
    assert pg.segments(pg.build(names, []), m._entries, total) == ([0], [0])
    assert len(begin) <= pg.MAX_SEGMENTS


def test_pairs_normalisation():
    assert pg.as_pairs(None) == [] and pg.as_pairs([]) == []
    assert pg.as_pairs([["*bias", {"lr": 0.1}]]) == [("*bias", {"lr": 0.1})]      # YAML: two-element lists are pairs
    with pytest.raises(ValueError):
        pg.as_pairs([("*bias",)])
    kw, pairs = optimizer_kwargs({"momentum": 0.9, "param_groups": [("*bias", {"lr": 0.1})]})
    assert kw == {"momentum": 0.9} and pairs == [("*bias", {"lr": 0.1})]
    assert optimizer_kwargs({"momentum": 0.9}) == ({"momentum": 0.9}, [])


@pytest.mark.parametrize("opt_cls, opt_kw, kind", [(SGD, {"momentum": 0.9}, "sgd"), (torch.optim.Adam, {}, "adam"),
                                                    (torch.optim.AdamW, {"weight_decay": 1e-2}, "adamw")])
def test_fused_kind_with_groups(opt_cls, opt_kw, kind):
    crit = CE(ignore_index=1)
    for settings in ({"lr": 1e-3}, {"weight_decay": 0.0}, {"lr": 1e-3, "weight_decay": 1e-4}):
        assert fused_kind(crit, opt_cls, opt_kw, _EngineModule, [("*bias", settings)]) == kind
    other = {"momentum": 0.5} if opt_cls is SGD else {"betas": (0.8, 0.9)}
    assert fused_kind(crit, opt_cls, opt_kw, _EngineModule, [("*bias", {"lr": 1e-3}), ("*norm*", other)]) is None
    assert fused_kind(crit, opt_cls, opt_kw, _EngineModule, [("*bias", {"eps": 1e-6} if opt_cls is not SGD else {"nesterov": True})]) is None
    assert fused_kind(crit, opt_cls, opt_kw, _EngineModule, []) == kind and fused_kind(crit, opt_cls, opt_kw, _EngineModule, None) == kind
    with pytest.raises(ValueError) as ours:
        fused_kind(crit, opt_cls, opt_kw, _EngineModule, [("*bias", {"weight_decay": -1.0})])
    with pytest.raises(ValueError) as torchs:
        opt_cls([torch.nn.Parameter(torch.zeros(1))], lr=0.01, **{**opt_kw, "weight_decay": -1.0})
    assert str(ours.value) == str(torchs.value)


@pytest.mark.parametrize("args", _table_test.pytestmark[0].args[1], ids=lambda a: f"{type(a[0]).__name__}-{a[1].__name__}-{a[2]}")
def test_fused_kind_table_still_holds_without_groups(args):
    crit, opt_cls, opt_kw, want = args
    assert fused_kind(crit, opt_cls, opt_kw, _EngineModule) == want
    assert fused_kind(crit, opt_cls, opt_kw, _EngineModule, []) == want


# ------------------------------------------------------------------------------------------------------------ schedules ----
BASE = [0.05, 0.02, 0.004]
# per-group forms of the arguments torch takes as lists
PER_GROUP = {"OneCycleLR": dict(max_lr=[0.1, 0.05, 0.01]), "CyclicLR": dict(base_lr=[0.01, 0.005, 0.001], max_lr=[0.1, 0.05, 0.01]),
             "LambdaLR": dict(lr_lambda=[lambda e: min(1.0, (e + 1) / 4), lambda e: 0.9 ** e, lambda e: 1.0])}


def torch_rows(policy, n, **kw):
    """Every group's rate before each of ``n`` optimizer steps on a real 3-group optimizer, the scheduler stepped after each."""
    opt = torch.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(2))], "lr": v} for v in BASE], lr=BASE[0])
    sch = getattr(torch.optim.lr_scheduler, policy)(opt, **kw)
    out = []
    for _ in range(n):
        out.append([g["lr"] for g in opt.param_groups])
        opt.step()
        sch.step()
    return out


@pytest.mark.parametrize("step_every", ["epoch", "batch"])
@pytest.mark.parametrize("policy", list(POLICIES))
def test_grouped_epoch_table_is_torch_own_sequence(policy, step_every):
    from slnlp.schedule import LRSchedule
    kw = {**POLICIES[policy], **PER_GROUP.get(policy, {})}
    total = N_EPOCHS * (N_BATCHES if step_every == "batch" else 1)
    want = torch_rows(policy, total, **kw)
    for k in range(N_EPOCHS):                                # k == 0: from the start; k > 0: after fast_forward
        s = LRSchedule(policy, BASE, step_every, **kw).fast_forward(fake_history(k))
        got = []
        for _ in range(N_EPOCHS - k):
            table = s.epoch_table(N_BATCHES)
            assert len(table) == N_BATCHES and all(len(row) == 3 and all(type(v) is float for v in row) for row in table)
            assert s.grouped
            got += table if step_every == "batch" else table[:1]
            if step_every == "epoch":
                assert all(row == table[0] for row in table)
                assert s.current == table[0][0] and s.current_all == table[0]     # what the history row reports: group 0's
            s.epoch_end()
        done = k * (N_BATCHES if step_every == "batch" else 1)
        assert got == want[done:], (policy, k)
    assert len(set(want[0])) == 3                                                  # the groups do differ


def test_one_group_schedule_keeps_its_float_rows():
    from slnlp.schedule import LRSchedule
    s = LRSchedule("StepLR", 0.05, "batch", step_size=2, gamma=0.5)
    assert not s.grouped and s.epoch_table(3) == [0.05, 0.05, 0.025] and s.rates == s.current


# ----------------------------------------------------------------------------------------------------------- checkpoint ----
class _HostNet:
    """The estimator's two checkpoint methods over a module whose arena is a CPU tensor: nothing here needs a GPU."""
    from slnlp.net import NeuralNetClassifier as _N
    _sgd_state_dict = _N._sgd_state_dict
    _load_sgd_state_dict = _N._load_sgd_state_dict
    _set_lr = _N._set_lr
    lrs_ = _N.lrs_

    def __init__(self, module, groups, lrs):
        self.module_, self._groups, self._fused, self._fused_kind = module, groups, True, "adamw"
        self._opt_cls, self._opt_kwargs, self.lr = torch.optim.AdamW, {"weight_decay": 1e-2}, 3e-3
        self._set_lr(lrs)


@pytest.mark.parametrize("which", ["tf", "gru"])
def test_checkpoint_maps_state_through_the_groups(which):
    m = make_module(which)
    named = list(m.named_parameters())
    groups = pg.build([n for n, _ in named], PAIRS)
    assert pg.positions(groups) != [n for n, _ in named]                           # the numbering really differs from named order
    lrs = [1e-3 * (i + 1) for i in range(len(groups))]
    net = _HostNet(m, groups, lrs)
    st = m._shared_state()
    # a recognisable fused-layout state: every float of the momentum / second-moment arenas is its own arena index
    n = m._arena.numel()
    st["momentum"].copy_(torch.arange(n, dtype=torch.float32))
    m.adam_second_moment().copy_(torch.arange(n, dtype=torch.float32) + 0.5)
    st["scalars"][2] = 7.0
    sd = net._sgd_state_dict()
    assert [g["lr"] for g in sd["param_groups"]] == lrs and len(sd["param_groups"]) == len(groups)
    # ... loads into the torch optimizer built from the same groups, every tensor on the parameter of the same name
    opt = torch.optim.AdamW(pg.torch_groups(groups, named), lr=3e-3, weight_decay=1e-2)
    opt.load_state_dict(sd)
    params = dict(named)
    ent = {name: (shape, off) for name, shape, off in m._entries}
    for name, p in params.items():
        if name in m._dead_params:
            assert p not in opt.state or not opt.state[p]
            continue
        shape, off = ent[name]
        want = torch.arange(off, off + p.numel(), dtype=torch.float32).view(*shape)
        assert torch.equal(opt.state[p]["exp_avg"], want), name
        assert torch.equal(opt.state[p]["exp_avg_sq"], want + 0.5), name
        assert float(opt.state[p]["step"]) == 7.0
    assert [g["lr"] for g in opt.param_groups] == lrs
    # and back: the torch optimizer's state_dict into a fresh fused layout
    m2 = make_module(which)
    net2 = _HostNet(m2, pg.build([n for n, _ in m2.named_parameters()], PAIRS), [0.0] * len(groups))
    net2._load_sgd_state_dict(opt.state_dict())
    st2 = m2._shared_state()
    live = torch.zeros(n, dtype=torch.bool)
    for name, shape, off in m2._entries:
        if name not in m2._dead_params:
            live[off:off + int(np.prod(shape))] = True
    assert torch.equal(st2["momentum"][live], st["momentum"][live])
    assert torch.equal(m2.adam_second_moment()[live], m.adam_second_moment()[live])
    assert float(st2["scalars"][2]) == 7.0 and net2.lrs_ == lrs and net2.lr_ == lrs[0]
    # a checkpoint written with other groups is refused, not mis-mapped
    other = _HostNet(m2, pg.build([n for n, _ in m2.named_parameters()], PAIRS[1:2]), [0.0, 0.0])     # "*bias" + the remainder
    with pytest.raises(ValueError, match="param groups"):
        other._load_sgd_state_dict(opt.state_dict())


# ----------------------------------------------------------------------------------------------------------------- grid ----
def test_candidates_differing_only_in_param_groups_share_a_lockstep_unit():
    y = np.repeat(np.arange(4), 10)
    param_grid = {"optimizer__param_groups": [[], [("*norm*", {"weight_decay": 0.0})], [("*bias", {"lr": 1e-3}), ("*norm*", {"lr": 1e-4})]],
                  "optimizer__weight_decay": [0.0, 1e-2]}
    cands, folds, tasks, order = grid.build_tasks(param_grid, y, 2)
    assert len(cands) == 6 and len(tasks) == 12
    units = grid.build_units(cands, folds, tasks, order, lockstep=16)
    assert len(units) == 1 and sorted(units[0]) == list(range(12))
    cands, folds, tasks, order = grid.build_tasks({**param_grid, "module__num_layers": [1, 2]}, y, 2)     # a shape key still splits
    assert len(grid.build_units(cands, folds, tasks, order, lockstep=32)) == 2


def test_cli_yaml_pairs_reach_the_estimator():
    from slnlp.cli import prefix_args
    p = prefix_args("optimizer", **{"weight_decay": 0.01, "param_groups": [["*norm*", {"weight_decay": 0.0}], ["*bias", {"lr": 0.001}]]})
    kw, pairs = optimizer_kwargs({k[len("optimizer__"):]: v for k, v in p.items()})
    assert kw == {"weight_decay": 0.01} and pairs == [("*norm*", {"weight_decay": 0.0}), ("*bias", {"lr": 0.001})]
