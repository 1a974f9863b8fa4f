"""GPU: ``optimizer__param_groups`` on the fused step -- the grouped update kernels against torch in fp64 and against the
one-group kernels bit for bit, the estimator's fused path against its torch-stepped path on the same groups, graph replay
against eager launches under a per-group schedule, lockstep groups of fits with different groups (and none) against their solo
fits, the grid search with the setting as an axis, and resume."""
import numpy as np
import pytest
import torch

from test_loss_optim_options_gpu import MODULES, PRE_OUT, make_net, rel, rnd

pytestmark = pytest.mark.gpu

N = 1 << 18
# 5 segments over 3 groups, boundaries on multiples of 4 (not of the block size), one skip range inside segment 1
SEG_BEGIN, SEG_GROUP = [0, 4100, 70000, 131072, 200004], [0, 1, 2, 0, 1]
GROUP_LR, GROUP_WD = [0.05, 0.01, 0.002], [1e-2, 0.0, 1e-3]
SKIP = (8192, 12288)


def group_slices():
    ends = SEG_BEGIN[1:] + [N]
    return [[(b, e) for b, e, g in zip(SEG_BEGIN, ends, SEG_GROUP) if g == gi] for gi in range(3)]


def torch_reference(opt_cls, p0, lrs, **kw):
    """fp64 parameters cut the way the table cuts the arena: one tensor per segment (the skip range its own tensors, which
    never get a gradient), grouped into 3 torch param groups."""
    cuts = sorted(set(SEG_BEGIN + [N, SKIP[0], SKIP[1]]))
    pieces = [(b, e, torch.nn.Parameter(p0[b:e].clone().double())) for b, e in zip(cuts, cuts[1:])]
    groups = []
    for gi, spans in enumerate(group_slices()):
        mine = [p for b, e, p in pieces if any(sb <= b and e <= se for sb, se in spans)]
        groups.append({"params": mine, "lr": lrs[gi], "weight_decay": GROUP_WD[gi]})
    return pieces, opt_cls(groups, **kw)


def ref_step(pieces, opt, g, max_norm=0.5):
    for b, e, p in pieces:
        p.grad = None if (SKIP[0] <= b and e <= SKIP[1]) else g[b:e].clone().double()
    total = torch.nn.utils.clip_grad_norm_([p for _, _, p in pieces], max_norm)
    opt.step()
    return total


def gather(pieces, opt=None, key=None):
    out = torch.zeros(N, dtype=torch.float64)
    for b, e, p in pieces:
        if key is None:
            out[b:e] = p.detach()
        elif p in opt.state and key in opt.state[p]:
            out[b:e] = opt.state[p][key]
    return out


def grads(step):
    g = rnd(N, seed=20 + step, scale=1e-2 if step % 2 else 1e-4)
    g[SKIP[0]:SKIP[1]] = 0.0                                            # a parameter that gets no gradient
    return g


# -------------------------------------------------------------------------------------------------------------- kernels ----
def test_clip_sgd_groups_plain_branch_vs_torch(monkeypatch):
    """No weight decay anywhere, no dampening, no Nesterov: the kernel's plain loop, with a different lr per group over 5 segments."""
    import sys
    monkeypatch.setattr(sys.modules[__name__], "GROUP_WD", [0.0, 0.0, 0.0])
    test_clip_sgd_groups_vs_torch({}, general=False)


@pytest.mark.parametrize("kw", [dict(), dict(nesterov=True), dict(dampening=0.3)], ids=["plain", "nesterov", "dampening"])
def test_clip_sgd_groups_vs_torch(kw, general=True):
    from slnlp import ops
    p0 = rnd(N, seed=1)
    assert any(GROUP_WD) == general
    table = ops.ParamGroupTable(N, SEG_BEGIN, SEG_GROUP, GROUP_WD)
    P, Bf, cnt = p0.cuda().clone(), torch.zeros(N, device="cuda"), torch.zeros(1, device="cuda")
    lr = torch.tensor(GROUP_LR, device="cuda")
    pieces, opt = torch_reference(torch.optim.SGD, p0, GROUP_LR, momentum=0.9, **kw)
    for step in range(5):
        g = grads(step)
        norm = ops.clip_sgd_step_groups(P, g.cuda(), Bf, table, lr, cnt, momentum=0.9, max_norm=0.5, skip=SKIP, **kw)
        total = ref_step(pieces, opt, g)
        e_norm, e_p, e_b = abs(float(norm) - float(total)) / float(total), rel(P, gather(pieces)), rel(Bf, gather(pieces, opt, "momentum_buffer"))
        print("sgd groups", kw, step, e_norm, e_p, e_b)
        assert e_norm < 1e-5
        assert e_p < 1e-6, step
        assert e_b < 1e-5, step
    assert float(cnt) == 5.0
    # (the plain loop steps the skip range too, like the one-group kernel: its gradient and buffer are zero, the weights stay)
    assert torch.equal(P[SKIP[0]:SKIP[1]].cpu(), p0[SKIP[0]:SKIP[1]]) and float(Bf[SKIP[0]:SKIP[1]].abs().max()) == 0.0


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_clip_adam_groups_vs_torch(decoupled):
    from slnlp import ops
    p0 = rnd(N, seed=1)
    lrs = [3e-3, 1e-3, 3e-4]
    table = ops.ParamGroupTable(N, SEG_BEGIN, SEG_GROUP, GROUP_WD)
    P, M1, M2 = p0.cuda().clone(), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    lr, cnt = torch.tensor(lrs, device="cuda"), torch.zeros(1, device="cuda")
    pieces, opt = torch_reference(torch.optim.AdamW if decoupled else torch.optim.Adam, p0, lrs, betas=(0.9, 0.99), eps=1e-8)
    live = torch.ones(N, dtype=torch.bool)
    if decoupled:
        live[SKIP[0]:SKIP[1]] = False          # plain Adam's fused update does not honour the skip range (as the one-group kernel)
    for step in range(5):
        g = grads(step)
        norm = ops.clip_adam_step_groups(P, g.cuda(), M1, M2, table, lr, cnt, betas=(0.9, 0.99), eps=1e-8, decoupled=decoupled,
                                         max_norm=0.5, skip=SKIP)
        total = ref_step(pieces, opt, g)
        e_norm = abs(float(norm) - float(total)) / float(total)
        e_p = float((P.cpu().double() - gather(pieces))[live].abs().max())
        e_m, e_v = rel(M1.cpu()[live], gather(pieces, opt, "exp_avg")[live]), rel(M2.cpu()[live], gather(pieces, opt, "exp_avg_sq")[live])
        print("adam groups", decoupled, step, e_norm, e_p, e_m, e_v)
        assert e_norm < 1e-5
        assert e_p < 1e-6 * (step + 1), step
        assert e_m < 1e-5 and e_v < 1e-5, step
    assert float(cnt) == 5.0
    if decoupled:
        assert torch.equal(P[SKIP[0]:SKIP[1]].cpu(), p0[SKIP[0]:SKIP[1]])


# the update's grid is capped at 2048 blocks of 256 float4: 1 << 18 floats is one trip of the grid-stride loop; the second size
# takes a second trip with a ragged tail, its skip range straddling the float4 index where that trip begins
ONE_GROUP_SIZES = {"one_trip": (1 << 18, (4096, 8192)), "two_trips": (4 * (2048 * 256 + 517), (4 * (2048 * 256 - 300), 4 * (2048 * 256 + 200)))}


@pytest.mark.parametrize("case,size", [pytest.param(c, s, id=c if s == "one_trip" else f"{c}-{s}")          # (the first size keeps its ids)
                                       for s in ONE_GROUP_SIZES for c in ("sgd_plain", "sgd_general", "adam", "adamw")])
def test_one_group_is_the_ungrouped_kernel_bit_for_bit(case, size):
    """One segment covering the arena with the fit's own lr / weight decay: weights and state equal the one-group entry point's."""
    from slnlp import ops
    n, skip = ONE_GROUP_SIZES[size]
    p0, b0, v0 = rnd(n, seed=1), rnd(n, seed=3, scale=1e-3), rnd(n, seed=4, scale=1e-3).abs()
    wd = {"sgd_plain": 0.0, "sgd_general": 1e-3, "adam": 1e-3, "adamw": 1e-2}[case]
    table = ops.ParamGroupTable(n, [0], [0], [wd])
    lr = torch.tensor([0.0371], device="cuda")
    a = dict(P=p0.cuda(), B=b0.cuda(), V=v0.cuda(), cnt=torch.zeros(1, device="cuda"))
    b = dict(P=p0.cuda(), B=b0.cuda(), V=v0.cuda(), cnt=torch.zeros(1, device="cuda"))
    for step in range(3):
        g = rnd(n, seed=30 + step, scale=1e-2 if step % 2 else 1e-4).cuda()
        if case == "sgd_plain":
            na = ops.clip_sgd_step_ex(a["P"], g, a["B"], lr, a["cnt"], momentum=0.9, max_norm=0.5)
            nb = ops.clip_sgd_step_groups(b["P"], g, b["B"], table, lr, b["cnt"], momentum=0.9, max_norm=0.5)
        elif case == "sgd_general":
            na = ops.clip_sgd_step_ex(a["P"], g, a["B"], lr, a["cnt"], momentum=0.9, dampening=0.3, weight_decay=wd, max_norm=0.5, skip=skip)
            nb = ops.clip_sgd_step_groups(b["P"], g, b["B"], table, lr, b["cnt"], momentum=0.9, dampening=0.3, max_norm=0.5, skip=skip)
        elif case == "adam":
            na = ops.clip_adam_step(a["P"], g, a["B"], a["V"], lr, a["cnt"], betas=(0.9, 0.99), weight_decay=wd, max_norm=0.5)
            nb = ops.clip_adam_step_groups(b["P"], g, b["B"], b["V"], table, lr, b["cnt"], betas=(0.9, 0.99), max_norm=0.5)
        else:
            na = ops.clip_adamw_step(a["P"], g, a["B"], a["V"], lr, a["cnt"], betas=(0.9, 0.99), weight_decay=wd, max_norm=0.5, skip=skip)
            nb = ops.clip_adam_step_groups(b["P"], g, b["B"], b["V"], table, lr, b["cnt"], betas=(0.9, 0.99), decoupled=True, max_norm=0.5, skip=skip)
        assert torch.equal(na, nb)
        for k in a:
            assert torch.equal(a[k], b[k]), (case, step, k)
    assert not torch.equal(a["P"].cpu(), p0)


def test_bad_tables_return_codes():
    from slnlp import ops
    for begin, group, wd in (([4, 8], [0, 1], [0.0, 0.0]),            # does not begin at 0
                             ([0, 6], [0, 1], [0.0, 0.0]),            # not a multiple of 4
                             ([0, 8, 8], [0, 1, 0], [0.0, 0.0]),      # not strictly increasing
                             ([0, 4096], [0, 1], [0.0, 0.0]),         # beyond the arena
                             ([0, 8], [0, 2], [0.0, 0.0]),            # group out of range
                             ([0, 8], [0, 1], [0.0, -1.0]),           # negative weight decay
                             (list(range(0, 4 * 1025, 4)), [i % 2 for i in range(1025)], [0.0, 0.0])):   # above the segment cap
        n = 4096 if len(begin) < 1000 else 8192
        with pytest.raises(RuntimeError):
            ops.ParamGroupTable(n, begin, group, wd)
    table = ops.ParamGroupTable(4096, [0, 8], [0, 1], [0.0, 0.0])
    z = lambda k=8192: torch.zeros(k, device="cuda")
    with pytest.raises(RuntimeError):                                   # an arena of another size than the table's
        ops.clip_sgd_step_groups(z(), z(), z(), table, torch.zeros(2, device="cuda"), torch.zeros(1, device="cuda"))


# ------------------------------------------------------------------------------------------------------------ estimator ----
GROUPS = [("*norm*", {"weight_decay": 0.0}), ("*bias*", {"weight_decay": 0.0, "lr": 0.02}), ("*embed*.weight", {"lr": 0.01})]
OPTS = {"sgd": dict(optimizer__weight_decay=1e-2), "adamw": dict(optimizer="torch.optim.AdamW", optimizer__weight_decay=1e-1, lr=3e-3)}


def adamw_groups():
    return [("*norm*", {"weight_decay": 0.0}), ("*bias*", {"weight_decay": 0.0, "lr": 1e-3}), ("*embed*.weight", {"lr": 1e-3})]


def groups_for(opt):
    return GROUPS if opt == "sgd" else adamw_groups()


def dataset():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(80, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


@pytest.mark.parametrize("opt", list(OPTS))
@pytest.mark.parametrize("module", list(MODULES))
def test_fused_equals_torch_stepped_path_on_the_same_groups(module, opt):
    from slnlp import param_groups as pg
    ds = dataset()
    nets = []
    for fused in (True, False):
        torch.manual_seed(11)
        net = make_net(ds, module, use_graph=False, optimizer__param_groups=groups_for(opt), **OPTS[opt]).initialize()
        assert net._fused and net._groups is not None and len(net._groups) == (4 if module == "tf" else 3)
        dead0 = net.module_.state_dict()[PRE_OUT].clone() if module != "tf" else None
        if not fused:                                   # force the stock-optimizer path around the autograd bridge
            net._fused, net._fused_kind = False, None
            net.optimizer_ = net._opt_cls(pg.torch_groups(net._groups, net.module_.named_parameters()), lr=net.lr, **net._opt_kwargs)
            assert [g["lr"] for g in net.optimizer_.param_groups] == net.lrs_
        net.partial_fit(ds)
        if dead0 is not None:
            assert torch.equal(net.module_.state_dict()[PRE_OUT], dead0)       # torch skips it: its grad is None
        nets.append(net)
    for key in ("train_loss", "valid_loss"):
        a, b = [h[key] for h in nets[0].history], [h[key] for h in nets[1].history]
        print(module, opt, key, max(abs(x - y) / abs(y) for x, y in zip(a, b)))
        assert np.allclose(a, b, rtol=1e-4), (key, a, b)
    assert [h["lr"] for h in nets[0].history] == [nets[0].lrs_[0]] * 3          # history lr: param_groups[0]'s


@pytest.mark.parametrize("opt", list(OPTS))
def test_the_table_is_not_ignored(opt):
    """weight_decay=0 on ``*norm*`` gives other final weights than the ungrouped fit; groups that only restate the defaults
    give the ungrouped fit's bits (the one-segment-per-group table against the one-group kernel, through the whole fit)."""
    ds = dataset()

    def fit(groups):
        torch.manual_seed(11)
        kw = {} if groups is None else {"optimizer__param_groups": groups}
        return make_net(ds, "tf", use_graph=False, **OPTS[opt], **kw).fit(ds)
    plain, nodecay = fit(None), fit([("*norm*", {"weight_decay": 0.0})])
    wd = OPTS[opt]["optimizer__weight_decay"]
    restated = fit([("*norm*", {"weight_decay": wd}), ("*bias", {"lr": plain.lr})])
    assert restated._groups is not None and len(restated._groups) == 3 and plain._groups is None
    sa, sb, sc = plain.module_.state_dict(), nodecay.module_.state_dict(), restated.module_.state_dict()
    norm_w = "transformer.encoder.layers.0.norm1.weight"
    assert not torch.equal(sa[norm_w], sb[norm_w])
    assert all(torch.equal(sa[k], sc[k]) for k in sa)
    assert [h["train_loss"] for h in plain.history] == [h["train_loss"] for h in restated.history]


def test_graph_replay_equals_eager_with_groups_and_a_per_group_schedule():
    ds = dataset()
    max_lr = [0.1, 0.04, 0.02, 0.05]
    sched = {"policy": "OneCycleLR", "step_every": "batch", "max_lr": max_lr, "total_steps": 12, "cycle_momentum": False}
    nets = []
    st = torch.cuda.Stream()
    for graph in (True, False):
        torch.manual_seed(11)
        with torch.cuda.stream(st):
            net = make_net(ds, "tf", use_graph=graph, optimizer__param_groups=GROUPS, lr_scheduler=sched, **OPTS["sgd"])
            nets.append(net.fit(ds))
    a, b = nets
    strip = lambda h: [{k: v for k, v in row.items() if k != "dur"} for row in h]
    assert strip(a.history) == strip(b.history)
    sa, sb = a.module_.state_dict(), b.module_.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    # event_lr: torch's group-0 rates on a real optimizer with the same groups
    opt = torch.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": v} for v in a._base_lrs()], lr=0.05)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=12, cycle_momentum=False)
    want = []
    for _ in range(12):
        want.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    got = [bt["event_lr"] for row in a.history for bt in row["batches"] if "event_lr" in bt]
    assert got == want and len(got) == 12


def test_set_param_groups_drops_captured_graphs():
    from slnlp import synth, tf_engine as te
    from slnlp._lib import load
    c = dict(Vs=64, Vt=16, E=32, H=4, N=2, F=64, B=4, S=12)
    X, _, y = [torch.from_numpy(a).cuda() for a in synth.make_batch(c["B"], c["S"], c["Vs"], c["Vt"], seed=1, min_len=3)]
    cfg = te.make_config(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"], c["B"], c["S"])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        eng = te.TransformerEngine(cfg, device="cuda:0")
        eng.params.normal_(0, 0.1)
        eng.set_lr(0.01)
        eng.train_step_graph(X, y)
        lr = torch.tensor([0.01, 0.02], device="cuda")
        eng.set_param_groups({"seg_begin": [0, 2048], "seg_group": [0, 1], "weight_decay": [0.0, 1e-2]}, lr)
        assert load().slnlp_tf_graph_launch(eng.handle, c["B"], st.cuda_stream) != 0
        eng.train_step_graph(X, y)
        eng.set_param_groups(None)
        assert load().slnlp_tf_graph_launch(eng.handle, c["B"], st.cuda_stream) != 0
        eng.train_step_graph(X, y)
    torch.cuda.synchronize()
    assert np.isfinite(eng.loss)
    with pytest.raises(RuntimeError):
        eng.set_param_groups({"seg_begin": [0, 2046], "seg_group": [0, 1], "weight_decay": [0.0, 0.0]}, lr)


def weight_planes(eng, lo=None, hi=None):
    """The bf16 hi / lo planes of the encoder layers' weights -- the range the update writes and the plane GEMMs read at B <= 64 --
    or of arena floats [lo, hi), as int16 views of the plan's workspace (``slnlp_tf_debug_layout`` names the offsets)."""
    import ctypes as C
    from slnlp import _lib
    buf = C.create_string_buffer(1 << 16)
    _lib.check(_lib.load().slnlp_tf_debug_layout(C.byref(eng.cfg), buf, len(buf)), "layout")
    at = dict((k, int(v)) for k, v in (line.split() for line in buf.value.decode().splitlines()))
    off = {name: o for name, _, o in eng.entries}
    lo = off["transformer.encoder.layers.0.self_attn.in_proj_weight"] if lo is None else lo
    hi = off["transformer.encoder.norm.weight"] if hi is None else hi
    planes = []
    for which in ("wp.hi", "wp.lo"):
        plane = eng.workspace[at[which]:at[which] + 2 * eng.arena_floats].view(torch.int16)
        planes.append(plane[lo:hi].clone())
    return planes


@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_one_segment_table_writes_the_ungrouped_weight_planes(kind):
    """Plan level: a one-segment table with the plan's own lr / weight decay against no table -- the arenas, the update's state
    and the bf16 hi / lo weight planes the update writes, bit for bit, after 3 steps.  E = F = 64: the plan runs on planes."""
    from slnlp import synth, tf_engine as te
    c = dict(Vs=64, Vt=16, E=64, H=4, N=2, F=64, B=4, S=12)
    X, _, y = [torch.from_numpy(a).cuda() for a in synth.make_batch(c["B"], c["S"], c["Vs"], c["Vt"], seed=1, min_len=3)]
    cfg = te.make_config(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"], c["B"], c["S"])
    wd = 1e-2
    engs = []
    for grouped in (False, True):
        eng = te.TransformerEngine(cfg, device="cuda:0")
        eng.params.copy_(rnd(eng.arena_floats, seed=2, scale=0.1).cuda())
        eng.set_lr(0.03)
        eng.set_update(kind=kind, weight_decay=wd)
        if grouped:
            lr = torch.tensor([0.03], device="cuda")
            eng.set_param_groups({"seg_begin": [0], "seg_group": [0], "weight_decay": [wd]}, lr)
        v2 = torch.zeros_like(eng.params)
        before = None
        for step in range(3):
            if kind == "sgd":
                eng.train_step(X, y)
            else:
                eng.train_step_adam(X, y, v2, weight_decay=wd)
            if step == 0:
                before = weight_planes(eng)
        torch.cuda.synchronize()
        engs.append((eng, v2, weight_planes(eng), before))
    (a, va, pa, pa0), (b, vb, pb, _) = engs
    assert torch.equal(a.params, b.params) and torch.equal(a.momentum, b.momentum) and torch.equal(va, vb)
    assert torch.equal(a.scalars, b.scalars)
    assert all(torch.equal(u, v) for u, v in zip(pa, pb))
    assert not torch.equal(pa[0], pa0[0]) and not torch.equal(pa[1], pa0[1])        # the update did rewrite both planes


# ----------------------------------------------------------------------------------------------------------- lockstep ----
def lock_variants(opt, module):
    """Two fits with different groups and one without."""
    norm = "*norm*" if module == "tf" else "*bridge*"
    g2 = [(norm, {"weight_decay": 0.0, "lr": 0.02 if opt == "sgd" else 1e-3})]
    return [dict(optimizer__param_groups=groups_for(opt)), dict(optimizer__param_groups=g2), dict()]


@pytest.mark.parametrize("sched", [None, "batch"], ids=["const", "per_batch"])
@pytest.mark.parametrize("opt", list(OPTS))
@pytest.mark.parametrize("module", ["tf", "gru"])
def test_lockstep_fits_with_different_groups_equal_solo_fits(module, opt, sched):
    from slnlp.data import synthetic_dataset
    from slnlp.lockstep import fit_lockstep, lockstep_supported
    ds = synthetic_dataset(150, seq_len=12, src_vocab=64, n_labels=6, seed=5, min_len=3)
    parts = [ds[np.arange(i * 5, i * 5 + 130)] for i in range(3)]
    extra = {}
    if sched:                                            # 104 train rows / 20: 6 batches x 3 epochs
        extra["lr_scheduler"] = {"policy": "OneCycleLR", "step_every": "batch", "max_lr": 0.1 if opt == "sgd" else 6e-3, "total_steps": 18,
                                 "cycle_momentum": False}

    def build():
        nets = []
        for i, kw in enumerate(lock_variants(opt, module)):
            torch.manual_seed(40 + i)
            nets.append(make_net(ds, module, use_graph=False, scoring=["neg_log_loss"], **OPTS[opt], **extra, **kw).initialize())
        return nets
    solo = build()
    for n, d in zip(solo, parts):
        n.partial_fit(d)
    lock = build()
    assert all(lockstep_supported(n) for n in lock)
    assert [None if n._groups is None else len(n._groups) for n in lock] == ([4, 2, None] if module == "tf" else [3, 2, None])
    fit_lockstep(lock, parts)
    strip = lambda h: [{k: v for k, v in row.items() if k != "dur"} for row in h]
    for a, b in zip(solo, lock):
        assert a._fused and strip(a.history) == strip(b.history)
        sa, sb = a.module_.state_dict(), b.module_.state_dict()
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert len({h["train_loss"] for h in (n.history[-1] for n in solo)}) == 3       # the settings did differ
    if sched:
        assert len({bt["event_lr"] for bt in solo[0].history[0]["batches"] if "event_lr" in bt}) > 1


@pytest.mark.parametrize("opt", list(OPTS))
@pytest.mark.parametrize("module", ["tf", "gru"])
def test_grid_with_param_groups_as_an_axis(module, opt, monkeypatch):
    """``optimizer__param_groups`` as a grid axis under ``lockstep=``: the candidates share a unit, the unit steps in lockstep (no
    one-at-a-time fallback inside it) and scores what the fits score one at a time."""
    from slnlp import grid as grid_mod
    from slnlp.data import synthetic_dataset
    from slnlp.grid import ShardedGridSearchCV
    ds = synthetic_dataset(100, seq_len=10, src_vocab=50, n_labels=3, seed=9, min_len=3)
    axis = {"optimizer__param_groups": [v.get("optimizer__param_groups", []) for v in lock_variants(opt, module)]}
    factory = lambda: make_net(ds, module, max_epochs=2, use_graph=False, scoring=["neg_log_loss"], **OPTS[opt])
    res = {1: ShardedGridSearchCV(factory, axis, cv=2, refit=False, device="cuda:0", lockstep=1).fit(ds)}
    one_at_a_time = []
    real = grid_mod.default_fit_and_score
    monkeypatch.setattr(grid_mod, "default_fit_and_score", lambda *a, **k: one_at_a_time.append(1) or real(*a, **k))
    res[6] = ShardedGridSearchCV(factory, axis, cv=2, refit=False, device="cuda:0", lockstep=6).fit(ds)
    assert not one_at_a_time                                          # every unit stepped in lockstep
    assert res[6].n_units_ <= 2 < res[1].n_units_ == 6              # (the unit builder may cut a unit under its memory / cost limits)
    for key in ("mean_test_score", "split0_test_score", "split1_test_score"):
        assert np.array_equal(res[1].cv_results_[key], res[6].cv_results_[key]), key
    assert len(set(res[1].cv_results_["mean_test_score"])) == 3


@pytest.mark.parametrize("module", ["tf", "gru"])
def test_checkpoint_resumes_and_loads_into_torch_adamw(module, tmp_path):
    from slnlp import param_groups as pg
    ds = dataset()
    kw = dict(optimizer__param_groups=adamw_groups(), **OPTS["adamw"])
    torch.manual_seed(3)
    full = make_net(ds, module, max_epochs=4, **kw).fit(ds)
    torch.manual_seed(3)
    first = make_net(ds, module, max_epochs=2, **kw).fit(ds)
    first.save_params(str(tmp_path))
    sd = torch.load(tmp_path / "optimizer.pt")
    named = list(first.module_.named_parameters())
    ref_opt = torch.optim.AdamW(pg.torch_groups(first._groups, named), lr=123.0)
    ref_opt.load_state_dict(sd)                                         # the stock optimizer built from the same groups accepts it
    assert [g["lr"] for g in ref_opt.param_groups] == first.lrs_ and ref_opt.param_groups[0]["weight_decay"] == 0.0
    mom = first.module_._shared_state()["momentum"]
    for name, shape, off in first.module_._entries:
        if name in first.module_._dead_params:
            continue
        buf = ref_opt.state[dict(named)[name]]["exp_avg"]
        assert torch.equal(buf.cpu(), mom[off:off + buf.numel()].view(*shape).cpu()), name
    torch.manual_seed(99)
    resumed = make_net(ds, module, max_epochs=2, warm_start=True, **kw).initialize()
    resumed.load_params(str(tmp_path))
    resumed.partial_fit(ds)
    assert [h["epoch"] for h in resumed.history] == [1, 2, 3, 4]
    for a, b in zip(resumed.history[2:], full.history[2:]):
        assert a["train_loss"] == pytest.approx(b["train_loss"], rel=1e-5), (a["train_loss"], b["train_loss"])
        assert a["valid_loss"] == pytest.approx(b["valid_loss"], rel=1e-5)
