"""GPU: CrossEntropyLoss(weight, label_smoothing, reduction) and SGD(dampening, weight_decay, nesterov) / AdamW on the fused
step -- kernels against torch, the estimator against its torch-stepped path, lockstep against solo fits, and resume."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    return o


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


# ------------------------------------------------------------------------------------------------------------ kernels ----
@pytest.mark.parametrize("B,V", [(1, 16), (50, 202), (1024, 202)])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.3])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_lsm_nll_ex_vs_torch(ops, B, V, weighted, eps, reduction):
    logits = rnd(B, V, seed=B + V, scale=2.0).double().requires_grad_(True)
    y = torch.randint(2, V, (B,), generator=torch.Generator().manual_seed(3))
    if B > 1:
        y[::7] = 1                                                       # ignored targets (== pad)
    w = (torch.rand(V, generator=torch.Generator().manual_seed(4)) + 0.25) if weighted else None
    logp_ref = torch.log_softmax(logits, -1)
    loss_ref = torch.nn.functional.cross_entropy(logp_ref, y, weight=None if w is None else w.double(), ignore_index=1,
                                                 label_smoothing=eps, reduction=reduction)
    loss_ref.backward()
    logp, loss, dl = ops.lsm_nll_ex(logits.detach().float().cuda(), y.cuda(), 1, weight=None if w is None else w.cuda(),
                                    label_smoothing=eps, reduction=reduction)
    assert rel(logp, logp_ref) < 1e-6
    assert abs(float(loss) - float(loss_ref)) < 1e-6 * abs(float(loss_ref)), (float(loss), float(loss_ref))
    assert rel(dl, logits.grad) < 1e-5
    # a batch whose every target is ignored: the mean is NaN (0 / 0, as torch), the sum 0; no gradient
    yp = torch.ones(B, dtype=torch.int64)
    _, loss, dl = ops.lsm_nll_ex(logits.detach().float().cuda(), yp.cuda(), 1, weight=None if w is None else w.cuda(),
                                 label_smoothing=eps, reduction=reduction)
    assert (np.isnan(float(loss)) if reduction == "mean" else float(loss) == 0.0)
    assert float(dl.abs().max()) == 0.0


def test_lsm_nll_ex_defaults_are_lsm_nll(ops):
    for B, V in ((1, 16), (50, 202), (1024, 202)):
        logits = rnd(B, V, seed=7, scale=2.0).cuda()
        y = torch.randint(1, V, (B,), generator=torch.Generator().manual_seed(8)).cuda()
        a, b = ops.lsm_nll(logits, y, 1), ops.lsm_nll_ex(logits, y, 1)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


SGD_CASES = [dict(nesterov=True), dict(dampening=0.3), dict(weight_decay=1e-2), dict(nesterov=True, weight_decay=1e-2)]


@pytest.mark.parametrize("kw", SGD_CASES, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_clip_sgd_ex_vs_torch(ops, kw):
    """Four steps against clip_grad_norm + torch.optim.SGD (fp64): the first step of dampening is undampened."""
    from oracle import train_ref
    n = 1 << 18
    p0 = rnd(n, seed=1)
    P, Bf, cnt = p0.cuda().clone(), torch.zeros(n, device="cuda"), torch.zeros(1, device="cuda")
    lr = torch.tensor([0.05], device="cuda")
    ref = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.SGD([ref], lr=0.05, momentum=0.9, **kw)
    for step in range(4):
        g = rnd(n, seed=20 + step, scale=1e-2 if step % 2 else 1e-4)
        norm = ops.clip_sgd_step_ex(P, g.cuda(), Bf, lr, cnt, momentum=0.9, max_norm=0.5, **kw)
        gg = [g.clone().double()]
        total, _ = train_ref.clip_grad_norm(gg, 0.5)
        ref.grad = gg[0]
        opt.step()
        assert abs(float(norm) - float(total)) < 1e-5 * float(total)
        assert rel(P, ref) < 1e-6, step
        assert rel(Bf, opt.state[ref]["momentum_buffer"]) < 1e-5, step
    assert float(cnt) == 4.0


def test_clip_sgd_ex_skip_range_and_defaults(ops):
    n = 1 << 16
    p0, g, b0 = rnd(n, seed=1), rnd(n, seed=2, scale=1e-3), rnd(n, seed=3, scale=1e-3)
    lr = torch.tensor([0.05], device="cuda")
    P, G, Bf, cnt = p0.cuda(), g.cuda(), b0.cuda(), torch.zeros(1, device="cuda")
    ops.clip_sgd_step_ex(P, G, Bf, lr, cnt, momentum=0.9, nesterov=True, weight_decay=1e-2, skip=(4096, 8192))
    assert torch.equal(P[4096:8192].cpu(), p0[4096:8192]) and torch.equal(Bf[4096:8192].cpu(), b0[4096:8192])
    assert not torch.equal(P[:4096].cpu(), p0[:4096]) and not torch.equal(P[8192:].cpu(), p0[8192:])
    # plain settings: the same bits as the SGD-momentum kernel
    P1, B1 = p0.cuda(), b0.cuda()
    P2, B2 = p0.cuda(), b0.cuda()
    ops.clip_sgd_step(P1, G, B1, lr, momentum=0.9, max_norm=0.5)
    ops.clip_sgd_step_ex(P2, G, B2, lr, torch.zeros(1, device="cuda"), momentum=0.9, max_norm=0.5)
    assert torch.equal(P1, P2) and torch.equal(B1, B2)


def test_clip_adamw_vs_torch(ops):
    n = 1 << 18
    p0 = rnd(n, seed=1)
    P, M1, M2 = p0.cuda().clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    lr, cnt = torch.tensor([3e-3], device="cuda"), torch.zeros(1, device="cuda")
    ref = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.AdamW([ref], lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
    for step in range(5):
        g = rnd(n, seed=10 + step, scale=1e-2 if step % 2 else 1e-4)
        g[1024:2048] = 0.0                                              # the skipped range: a parameter that gets no gradient
        norm = ops.clip_adamw_step(P, g.cuda(), M1, M2, lr, cnt, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, max_norm=0.5,
                                   skip=(1024, 2048))
        ref.grad = g.clone().double()
        total = torch.nn.utils.clip_grad_norm_([ref], 0.5)
        with torch.no_grad():
            keep = ref[1024:2048].clone()
        opt.step()
        with torch.no_grad():
            ref[1024:2048] = keep                                       # torch skips a parameter whose grad is None
        assert abs(float(norm) - float(total)) < 1e-5 * float(total)
        assert float((P.cpu().double() - ref.detach()).abs().max()) < 1e-6 * (step + 1), step
    assert torch.equal(P[1024:2048].cpu(), p0[1024:2048])
    assert float(cnt) == 5.0


# ---------------------------------------------------------------------------------------------------------- estimator ----
CFG = dict(module__embedding_size=32, module__num_heads=4, module__num_layers=2, module__hidden_size=64)
RNN_CFG = dict(module__embedding_size=24, module__hidden_size=32, module__num_layers=2)
MODULES = {"tf": ("model.Transformer", CFG), "lstm": ("model.EncoderDecoderLSTMAttn", RNN_CFG),
           "gru": ("model.EncoderDecoderGRUAttn", RNN_CFG)}
OPTIONS = {
    "smoothing": dict(criterion__label_smoothing=0.1),
    "weights": dict(criterion__weight="random"),
    "nesterov_wd": dict(optimizer__nesterov=True, optimizer__weight_decay=1e-3),
    "dampening": dict(optimizer__dampening=0.5),
    "adamw": dict(optimizer="torch.optim.AdamW", optimizer__weight_decay=1e-2, lr=3e-3),
}
PRE_OUT = "model.decoder.pre_output_layer.weight"


def make_net(ds, module="tf", **kw):
    from slnlp.net import NeuralNetClassifier
    mod, cfg = MODULES[module]
    args = dict(module=mod, module__dropout=0.0, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y,
                module__batch_first=True, **cfg, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1,
                optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05, max_epochs=3, batch_size=20, device="cuda",
                gradient_clipping={"gradient_clip_value": 0.5})
    if kw.get("criterion__weight") == "random":
        kw["criterion__weight"] = torch.rand(len(ds.vocab_y), generator=torch.Generator().manual_seed(5)) + 0.5
    if kw.get("optimizer") in ("torch.optim.Adam", "torch.optim.AdamW"):
        args.pop("optimizer__momentum")
    args.update(kw)
    return NeuralNetClassifier(**args)


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("module", list(MODULES))
def test_fused_equals_torch_stepped_path(module, option):
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(80, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)
    nets = []
    for fused in (True, False):
        torch.manual_seed(11)
        net = make_net(ds, module, use_graph=False, **OPTIONS[option]).initialize()
        assert net._fused
        dead0 = net.module_.state_dict()[PRE_OUT].clone() if module != "tf" else None
        if not fused:                                   # force the stock-optimizer path around the autograd bridge
            net._fused, net._fused_kind = False, None
            net.optimizer_ = net._opt_cls(net.module_.parameters(), lr=net.lr, **net._opt_kwargs)
        net.partial_fit(ds)
        if dead0 is not None and ("weight_decay" in str(OPTIONS[option]) or option == "adamw"):
            assert torch.equal(net.module_.state_dict()[PRE_OUT], dead0)       # torch skips it: its grad is None
        nets.append(net)
    for key in ("train_loss", "valid_loss"):
        a, b = [h[key] for h in nets[0].history], [h[key] for h in nets[1].history]
        print(module, option, key, max(abs(x - y) / abs(y) for x, y in zip(a, b)))
        assert np.allclose(a, b, rtol=1e-4), (key, a, b)


def test_setting_change_drops_captured_graphs():
    """A criterion / update change after a graph capture drops the plan's graphs: the old one is gone, the engine re-captures."""
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
        plain = eng.loss
        eng.set_criterion(label_smoothing=0.2)
        assert load().slnlp_tf_graph_launch(eng.handle, c["B"], st.cuda_stream) != 0
        eng.train_step_graph(X, y)
        smoothed = eng.loss
        eng.set_criterion(label_smoothing=0.2)          # no change: the new graph stays
        assert load().slnlp_tf_graph_launch(eng.handle, c["B"], st.cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.isfinite(plain) and np.isfinite(smoothed) and smoothed != plain
    with pytest.raises(ValueError):
        eng.set_criterion(weight=torch.ones(5))


# ----------------------------------------------------------------------------------------------------------- lockstep ----
LOCK_VARIANTS = [dict(criterion__label_smoothing=0.0), dict(criterion__label_smoothing=0.1),
                 dict(optimizer__weight_decay=1e-3, optimizer__dampening=0.3), dict(optimizer__nesterov=True, optimizer__weight_decay=1e-4)]


@pytest.mark.parametrize("module", ["tf", "lstm"])
def test_lockstep_fits_with_own_settings_equal_solo_fits(module):
    from slnlp.data import synthetic_dataset
    from slnlp.lockstep import fit_lockstep
    ds = synthetic_dataset(150, seq_len=12, src_vocab=64, n_labels=6, seed=5, min_len=3)
    parts = [ds[np.arange(i * 5, i * 5 + 130)] for i in range(4)]

    def build():
        nets = []
        for i, kw in enumerate(LOCK_VARIANTS):
            torch.manual_seed(40 + i)
            nets.append(make_net(ds, module, use_graph=False, scoring=["neg_log_loss"], **kw).initialize())
        return nets
    solo = build()
    for n, d in zip(solo, parts):
        n.partial_fit(d)
    lock = build()
    fit_lockstep(lock, parts)
    strip = lambda h: [{k: v for k, v in row.items() if k != "dur"} for row in h]
    for a, b in zip(solo, lock):
        assert a._fused and strip(a.history) == strip(b.history)
        sa, sb = a.module_.state_dict(), b.module_.state_dict()
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert len({h["train_loss"] for h in (n.history[-1] for n in solo)}) == 4      # the settings did differ


@pytest.mark.parametrize("optimizer", ["sgd", "adam", "adamw"])
def test_sharded_grid_lockstep_over_per_fit_settings(optimizer, monkeypatch):
    """Candidates that differ only in per-fit settings share a unit AND run it in lockstep (no one-at-a-time fallback inside
    the unit); cv_results_ equal lockstep=1's."""
    from slnlp import grid as grid_mod
    from slnlp.data import synthetic_dataset
    from slnlp.grid import ShardedGridSearchCV
    ds = synthetic_dataset(100, seq_len=10, src_vocab=50, n_labels=3, seed=9, min_len=3)
    if optimizer == "sgd":
        grid = {"criterion__label_smoothing": [0.0, 0.1], "optimizer__weight_decay": [0.0, 1e-3], "optimizer__nesterov": [False, True]}
        opt = {}
    else:
        grid = {"criterion__label_smoothing": [0.0, 0.1], "optimizer__weight_decay": [0.0, 1e-3, 1e-2, 3e-2]}
        opt = dict(OPTIONS["adamw"], optimizer="torch.optim.AdamW" if optimizer == "adamw" else "torch.optim.Adam")
        opt.pop("optimizer__weight_decay")
    factory = lambda: make_net(ds, max_epochs=2, use_graph=False, scoring=["neg_log_loss"], **opt)
    res = {1: ShardedGridSearchCV(factory, grid, cv=2, refit=False, device="cuda:0", lockstep=1).fit(ds)}
    one_at_a_time = []
    real = grid_mod.default_fit_and_score
    monkeypatch.setattr(grid_mod, "default_fit_and_score", lambda *a, **k: one_at_a_time.append(1) or real(*a, **k))
    res[4] = ShardedGridSearchCV(factory, grid, cv=2, refit=False, device="cuda:0", lockstep=4).fit(ds)
    assert not one_at_a_time                                          # every unit stepped in lockstep
    assert res[4].n_units_ <= 4 < res[1].n_units_ == 16
    for key in ("mean_test_score", "split0_test_score", "split1_test_score"):
        assert np.array_equal(res[1].cv_results_[key], res[4].cv_results_[key]), key


@pytest.mark.parametrize("optimizer", ["torch.optim.Adam", "torch.optim.AdamW"])
def test_lockstep_adam_fits_with_own_weight_decay_equal_solo_fits(optimizer):
    from slnlp.data import synthetic_dataset
    from slnlp.lockstep import _adam_key, fit_lockstep
    ds = synthetic_dataset(150, seq_len=12, src_vocab=64, n_labels=6, seed=5, min_len=3)
    parts = [ds[np.arange(i * 5, i * 5 + 130)] for i in range(3)]

    def build():
        nets = []
        for i, wd in enumerate((0.0, 1e-3, 3e-2)):
            torch.manual_seed(50 + i)
            nets.append(make_net(ds, use_graph=False, scoring=["neg_log_loss"], optimizer=optimizer, optimizer__weight_decay=wd,
                                 lr=3e-3).initialize())
        return nets
    solo = build()
    for n, d in zip(solo, parts):
        n.partial_fit(d)
    lock = build()
    assert len({_adam_key(n) for n in lock}) == 1
    fit_lockstep(lock, parts)
    strip = lambda h: [{k: v for k, v in row.items() if k != "dur"} for row in h]
    for a, b in zip(solo, lock):
        assert strip(a.history) == strip(b.history)
        sa, sb = a.module_.state_dict(), b.module_.state_dict()
        assert all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("option", ["dampening", "nesterov_wd", "smoothing"])
@pytest.mark.parametrize("module", ["tf", "lstm"])
def test_graph_replay_equals_eager_steps(module, option):
    """The captured-graph step (whose replays advance the device-side SGD step count) gives the eager step's bits."""
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(80, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)
    nets = []
    for graph in (True, False):
        torch.manual_seed(11)
        nets.append(make_net(ds, module, use_graph=graph, **OPTIONS[option]).fit(ds))
    strip = lambda h: [{k: v for k, v in row.items() if k != "dur"} for row in h]
    assert strip(nets[0].history) == strip(nets[1].history)
    sa, sb = nets[0].module_.state_dict(), nets[1].module_.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------------------------------------------------- resume ----
@pytest.mark.parametrize("option", ["dampening", "adamw"])
def test_resume_equals_uninterrupted_fit(tmp_path, option):
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(100, seq_len=10, src_vocab=50, n_labels=5, seed=8, min_len=3)
    kw = dict(OPTIONS[option], use_graph=False)
    torch.manual_seed(3)
    full = make_net(ds, max_epochs=4, **kw).fit(ds)
    torch.manual_seed(3)
    first = make_net(ds, max_epochs=2, **kw).fit(ds)
    first.save_params(str(tmp_path))
    sd = torch.load(tmp_path / "optimizer.pt")
    if option == "adamw":
        ref = torch.optim.AdamW(first.module_.parameters(), lr=1.0, weight_decay=1e-2)
    else:
        ref = torch.optim.SGD(first.module_.parameters(), lr=1.0, momentum=0.9, dampening=0.5)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["lr"] == pytest.approx(first.lr_)
    assert all(not torch.is_tensor(v) or v.device.type == "cpu" for v in torch.load(tmp_path / "criterion.pt").values())
    torch.manual_seed(99)
    resumed = make_net(ds, max_epochs=2, warm_start=True, **kw).initialize()
    resumed.load_params(str(tmp_path))
    resumed.partial_fit(ds)
    # (valid_loss_best is relative to the epochs the fit itself has seen: not part of the comparison)
    strip = lambda h: [{k: row[k] for k in ("epoch", "train_loss", "valid_loss", "lr", "batches")} for row in h]
    assert strip(resumed.history[2:]) == strip(full.history[2:])
    sa, sb = resumed.module_.state_dict(), full.module_.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
