"""GPU: shuffled train batches (``iterator_train__shuffle`` / ``iterator_train__drop_last``) on every fit path, pinned by
bit-equality: the gather launch against ``index_select`` on the host, a shuffled fit against one-epoch fits on datasets
permuted ON THE HOST by the orders torch's own sampler yields, lockstep order tables against solo fits, the torch-stepped
path, the grid, resume, and the argument errors of ``set_order``.

The Transformer case is bench.py's cfg1 shape with dropout 0.1: 170 rows of length 48, batch 50 -> four train batches per
epoch, the last one of 20 rows; with drop_last three batches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG1 = dict(module__embedding_size=128, module__num_heads=4, module__num_layers=2, module__hidden_size=256)
SMALL = dict(module__embedding_size=32, module__num_heads=4, module__num_layers=2, module__hidden_size=64)
RNN_CFG = dict(module__embedding_size=24, module__hidden_size=32, module__num_layers=2)
MODULES = {"tf": ("model.Transformer", CFG1), "tf_small": ("model.Transformer", SMALL), "lstm": ("model.EncoderDecoderLSTMAttn", RNN_CFG),
           "gru": ("model.EncoderDecoderGRUAttn", RNN_CFG)}
N, BS = 170, 50
SHUFFLE = dict(iterator_train__shuffle=True)


def dataset(n=N, module="tf"):
    from slnlp.data import synthetic_dataset
    if module == "tf":
        return synthetic_dataset(n, seq_len=48, src_vocab=3000, n_labels=200, seed=6, min_len=8)
    return synthetic_dataset(n, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


def make_net(ds, module="tf", **kw):
    from slnlp.net import NeuralNetClassifier
    mod, cfg = MODULES[module]
    args = dict(module=mod, module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y,
                module__batch_first=True, **cfg, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1,
                optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05, max_epochs=3, batch_size=BS, device="cuda",
                gradient_clipping={"gradient_clip_value": 0.5}, train_split=None)
    if kw.get("optimizer", "torch.optim.SGD") != "torch.optim.SGD":
        args.pop("optimizer__momentum")
    args.update(kw)
    return NeuralNetClassifier(**args)


def strip(history):
    return [{k: v for k, v in row.items() if k != "dur"} for row in history]


def same_weights(a, b):
    sa, sb = a.module_.state_dict(), b.module_.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


def momentum(net):
    return net.module_._shared_state()["momentum"]


def batch_losses(net):
    return [[b["train_loss"] for b in row["batches"] if "train_loss" in b] for row in net.history]


def host_permuted_reference(ds, module, seed, shuffle_seed, epochs, drop_last=False, bs=BS, **kw):
    """The definition of a shuffled fit: an UNSHUFFLED estimator under the same torch seed, one ``partial_fit`` of one epoch per
    epoch, each on the dataset permuted (and, with drop_last, truncated) on the host by torch's own sampler."""
    from slnlp.sampler import EpochOrder
    torch.manual_seed(seed)
    ref = make_net(ds, module, max_epochs=1, batch_size=bs, **kw).initialize()
    orders = EpochOrder(len(ds), bs, shuffle_seed, drop_last)
    for _ in range(epochs):
        ref.partial_fit(ds[orders.next_epoch()])
    return ref


# ----------------------------------------------------------------------------------------------------- the launch ----
@pytest.mark.parametrize("S", [1, 48, 65])
def test_gather_batch_equals_index_select_on_the_host(S):
    from slnlp import ops
    rows, B = 137, 50
    rng = np.random.RandomState(S)
    X = torch.from_numpy(rng.randint(0, 3000, (rows, S)).astype(np.int64))
    L = torch.from_numpy(rng.randint(1, S + 1, rows).astype(np.int64))
    y = torch.from_numpy(rng.randint(0, 202, rows).astype(np.int64))
    order = torch.from_numpy(rng.permutation(rows).astype(np.int64))
    Xd, Ld, yd, od = X.cuda(), L.cuda(), y.cuda(), order.cuda()
    for row0, b in [(0, B), (50, B), (100, 37), (136, 1)]:                      # first / middle / short last batch / one row
        for use_order in (True, False):
            idx = order[row0:row0 + b] if use_order else torch.arange(row0, row0 + b)
            for with_len in (True, False):
                xb, lb, yb = ops.gather_batch(Xd, Ld if with_len else None, yd, od if use_order else None, row0, b)
                torch.cuda.synchronize()
                assert torch.equal(xb.cpu(), X.index_select(0, idx)) and torch.equal(yb.cpu(), y.index_select(0, idx))
                assert (lb is None) if not with_len else torch.equal(lb.cpu(), L.index_select(0, idx))
    # into given staging buffers larger than the batch: only the batch's rows are written
    stage = (torch.full((B, S), -7, dtype=torch.int64, device="cuda"), torch.full((B,), -7, dtype=torch.int64, device="cuda"),
             torch.full((B,), -7, dtype=torch.int64, device="cuda"))
    xb, lb, yb = ops.gather_batch(Xd, Ld, yd, od, 100, 37, out=stage)
    torch.cuda.synchronize()
    assert xb.data_ptr() == stage[0].data_ptr() and torch.equal(xb.cpu(), X.index_select(0, order[100:137]))
    assert bool((stage[0][37:] == -7).all()) and bool((stage[1][37:] == -7).all()) and bool((stage[2][37:] == -7).all())
    with pytest.raises(ValueError):
        ops.gather_batch(Xd, Ld, yd, od, 100, 38)                              # past the order's end: checked on the host


def test_gather_batch_argument_errors_are_codes():
    from slnlp._lib import load, ptr
    lib = load()
    t = torch.zeros(4, 3, dtype=torch.int64, device="cuda")
    v = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.slnlp_gather_batch(ptr(t), None, ptr(v), None, 0, 4, 3, None, None, ptr(v), st) == 1      # NULL X_out
    assert lib.slnlp_gather_batch(ptr(t), None, ptr(v), None, 0, 4, 3, ptr(t), None, None, st) == 1      # NULL y_out
    assert lib.slnlp_gather_batch(ptr(t), ptr(v), ptr(v), None, 0, 4, 3, ptr(t), None, ptr(v), st) == 1  # lengths without len_out
    assert lib.slnlp_gather_batch(ptr(t), None, ptr(v), None, 0, 0, 3, ptr(t), None, ptr(v), st) == 1    # B = 0
    assert lib.slnlp_gather_batch(ptr(t), None, ptr(v), None, -1, 4, 3, ptr(t), None, ptr(v), st) == 1   # row0 < 0
    assert b"gather_batch" in lib.slnlp_last_error()


# ------------------------------------------------------------------------------------------------ the estimator ----
@pytest.mark.parametrize("drop_last", [False, True], ids=["all_rows", "drop_last"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("module", ["tf", "lstm"])
def test_a_shuffled_fit_is_one_epoch_fits_on_host_permuted_data(module, graph, drop_last):
    ds = dataset(module=module)
    kw = dict(use_graph=graph)
    torch.manual_seed(21)
    net = make_net(ds, module, iterator_train__shuffle=True, iterator_train__drop_last=drop_last, **kw).fit(ds)
    assert net._fused and isinstance(net.shuffle_seed_, int)
    assert all(row["shuffle_seed"] == net.shuffle_seed_ for row in net.history)
    ref = host_permuted_reference(ds, module, 21, net.shuffle_seed_, 3, drop_last, **kw)
    assert all("shuffle_seed" not in row for row in ref.history)
    sizes = [[b["train_batch_size"] for b in row["batches"]] for row in net.history]
    assert sizes == [[50, 50, 50] if drop_last else [50, 50, 50, 20]] * 3
    assert batch_losses(net) == batch_losses(ref)
    assert [r["train_loss"] for r in net.history] == [r["train_loss"] for r in ref.history]
    assert same_weights(net, ref) and torch.equal(momentum(net), momentum(ref))


@pytest.mark.parametrize("module", ["tf", "lstm"])
def test_shuffling_changes_the_fit(module):
    ds = dataset(module=module)
    nets = []
    for shuffle in (True, False):
        torch.manual_seed(21)
        nets.append(make_net(ds, module, use_graph=False, max_epochs=1, iterator_train__shuffle=shuffle).fit(ds))
    a, b = batch_losses(nets[0])[0], batch_losses(nets[1])[0]
    assert len(a) == len(b) == 4 and a != b
    assert not same_weights(*nets)
    assert nets[1].shuffle_seed_ is None and "shuffle_seed" not in nets[1].history[0]


@pytest.mark.parametrize("init", ["reference", "recipe"])
@pytest.mark.parametrize("module", ["tf_small", "gru"])
def test_the_seed_draw_does_not_move_the_weights(module, init):
    ds = dataset(module=module)
    nets = []
    for shuffle in (True, False, True):
        torch.manual_seed(8)
        nets.append(make_net(ds, module, module__init=init, iterator_train__shuffle=shuffle).initialize())
    assert same_weights(nets[0], nets[1]) and same_weights(nets[0], nets[2])
    assert nets[0].shuffle_seed_ == nets[2].shuffle_seed_ and nets[1].shuffle_seed_ is None
    torch.manual_seed(9)
    assert make_net(ds, module, module__init=init, **SHUFFLE).initialize().shuffle_seed_ != nets[0].shuffle_seed_


def test_train_scores_pair_the_log_probs_with_the_labels_in_visit_order():
    """Epoch metrics of a shuffled fit against sklearn on what the fit itself saw: the reference estimator of the host-permuted
    data scores its (dataset-order) train log-probs against the permuted labels."""
    ds = dataset(module="lstm")
    scoring = ["accuracy", "neg_log_loss", "f1_weighted", "precision_macro"]                 # the last one takes the sklearn path
    torch.manual_seed(4)
    net = make_net(ds, "lstm", use_graph=False, scoring=scoring, **SHUFFLE).fit(ds)
    ref = host_permuted_reference(ds, "lstm", 4, net.shuffle_seed_, 3, use_graph=False, scoring=scoring)
    for a, b in zip(net.history, ref.history):
        for s in scoring:
            assert a[f"train_{s}"] == b[f"train_{s}"], s
    assert len({row["train_accuracy"] for row in net.history}) > 1


def test_drop_last_without_a_full_batch_is_an_error_at_fit_start():
    ds = dataset(30, "lstm")
    net = make_net(ds, "lstm", iterator_train__drop_last=True).initialize()
    with pytest.raises(ValueError, match="drop_last"):
        net.partial_fit(ds)
    assert net.history == []


def test_torch_stepped_path_takes_the_same_order():
    ds = dataset(module="lstm")
    kw = dict(optimizer="torch.optim.RMSprop", lr=1e-3, module__dropout=0.0)
    torch.manual_seed(13)
    net = make_net(ds, "lstm", **SHUFFLE, **kw).fit(ds)
    assert not net._fused
    ref = host_permuted_reference(ds, "lstm", 13, net.shuffle_seed_, 3, **kw)
    assert batch_losses(net) == batch_losses(ref) and same_weights(net, ref)
    torch.manual_seed(13)
    plain = make_net(ds, "lstm", **kw).fit(ds)
    assert batch_losses(plain)[0] != batch_losses(net)[0]


# ------------------------------------------------------------------------------------------------------ lockstep ----
@pytest.mark.parametrize("module", ["tf_small", "gru"])
def test_identity_order_table_changes_nothing(module):
    from slnlp.lockstep import LockstepGroup, TRAIN
    ds = dataset(64, module)
    K, bs = 3, 20
    out = []
    for with_order in (False, True):
        nets = []
        for s in (31, 32, 33):
            torch.manual_seed(s)
            nets.append(make_net(ds, module, batch_size=bs).initialize())
        st = nets[0]._stream
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            engines = [n.module_.engine(bs, ds.ids.shape[1]) for n in nets]
            X, L, y = nets[0]._device_data(ds)
            for e in engines:
                e.set_lr(0.05)
            grp = LockstepGroup(engines)
            grp.set_data(TRAIN, [X] * K, [y] * K, bs, [L] * K)
            if with_order:
                ident = torch.arange(64, dtype=torch.int64, device=X.device)
                grp.set_order(TRAIN, [ident, ident.clone(), None])
            grp.epoch(TRAIN, bs, True, 0.9, 0.5)
            st.synchronize()
            out.append(([lp.clone() for lp in grp.logp[TRAIN]], [l.clone() for l in grp.loss[TRAIN]], [e.params.clone() for e in engines],
                        (grp.num_launches(TRAIN, bs, True), grp.num_launches(TRAIN, 4, True))))
            if with_order:                                # clearing the order drops no program either
                grp.set_order(TRAIN, None)
                assert (grp.num_launches(TRAIN, bs, True), grp.num_launches(TRAIN, 4, True)) == out[0][3]
            grp.close()
    (lp0, l0, p0, n0), (lp1, l1, p1, n1) = out
    assert n0 == n1 and min(n0) > 0
    for f in range(K):
        assert torch.equal(lp0[f], lp1[f]) and torch.equal(l0[f], l1[f]) and torch.equal(p0[f], p1[f]), f


@pytest.mark.parametrize("module,opt", [("tf_small", "sgd"), ("lstm", "sgd"), ("tf_small", "adam")])
def test_lockstep_fits_with_own_orders_equal_solo_fits(module, opt):
    """Two shuffled fits (own seeds; one with a per-batch OneCycleLR), one unshuffled, one that EarlyStopping takes out of the
    group mid-run -- so the order tables are re-sent to the regrouped fits -- each bit-equal to its solo fit."""
    from slnlp.lockstep import fit_lockstep
    ds = dataset(100, module)
    parts = [ds[np.arange(i * 5, i * 5 + 80)] for i in range(4)]
    epochs, bs = 5, 20
    onecycle = {"policy": "OneCycleLR", "step_every": "batch", "max_lr": 0.1, "total_steps": epochs * 4, "cycle_momentum": False}
    stop = {"patience": 2, "threshold": 10.0, "threshold_mode": "abs"}          # no epoch after the first can meet it
    settings = [dict(SHUFFLE), dict(SHUFFLE, lr_scheduler=onecycle), dict(), dict(SHUFFLE, early_stopping=stop)]
    extra = dict(optimizer="torch.optim.Adam", lr=3e-3) if opt == "adam" else {}
    if opt == "adam":
        settings[1]["lr_scheduler"] = dict(onecycle, max_lr=1e-2)

    def build():
        nets = []
        for i, kw in enumerate(settings):
            torch.manual_seed(40 + i)
            nets.append(make_net(ds, module, use_graph=False, scoring=["neg_log_loss", "accuracy"], max_epochs=epochs, batch_size=bs,
                                 train_split=5, **extra, **kw).initialize())
        return nets
    solo = build()
    for n, d in zip(solo, parts):
        n.partial_fit(d)
    lock = build()
    fit_lockstep(lock, parts)
    for a, b in zip(solo, lock):
        assert a._fused and a.shuffle_seed_ == b.shuffle_seed_
        assert strip(a.history) == strip(b.history)
        assert same_weights(a, b)
    assert [len(n.history) for n in lock] == [epochs, epochs, epochs, 3]
    seeds = [n.shuffle_seed_ for n in lock]
    assert seeds[2] is None and len({seeds[0], seeds[1], seeds[3]}) == 3


def test_lockstep_drop_last_visits_the_full_batches_only():
    from slnlp.lockstep import fit_lockstep
    ds = dataset(100, "gru")
    parts = [ds[np.arange(i * 5, i * 5 + 70)] for i in range(3)]
    settings = [dict(SHUFFLE), dict(), dict(SHUFFLE)]

    def build():
        nets = []
        for i, kw in enumerate(settings):
            torch.manual_seed(50 + i)
            nets.append(make_net(ds, "gru", use_graph=False, scoring=["accuracy"], max_epochs=2, batch_size=20, iterator_train__drop_last=True,
                                 **kw).initialize())
        return nets
    solo = build()
    for n, d in zip(solo, parts):
        n.partial_fit(d)
    lock = build()
    fit_lockstep(lock, parts)
    for a, b in zip(solo, lock):
        assert strip(a.history) == strip(b.history) and same_weights(a, b)
        assert [bt["train_batch_size"] for bt in b.history[0]["batches"]] == [20, 20, 20]
    ref = host_permuted_reference(parts[0], "gru", 50, lock[0].shuffle_seed_, 2, drop_last=True, bs=20, use_graph=False)
    assert batch_losses(lock[0]) == batch_losses(ref) and same_weights(lock[0], ref)


def test_set_order_argument_errors():
    from slnlp.lockstep import LockstepGroup, TRAIN, VALID
    ds = dataset(64, "gru")
    torch.manual_seed(1)
    net = make_net(ds, "gru", batch_size=20).initialize()
    with torch.cuda.stream(net._stream):
        eng = net.module_.engine(20, ds.ids.shape[1])
        X, L, y = net._device_data(ds)
        grp = LockstepGroup([eng])
        ident = torch.arange(64, dtype=torch.int64, device=X.device)
        with pytest.raises(RuntimeError, match="no data"):
            grp.set_order(TRAIN, [ident])
        grp.set_data(TRAIN, [X], [y], 20, [L])
        for bad in (0, 65):
            with pytest.raises(RuntimeError, match="n_visit"):
                grp.set_order(TRAIN, [None], bad)
        with pytest.raises(RuntimeError, match="no data"):
            grp.set_order(VALID, [ident])
        with pytest.raises(RuntimeError, match="slot"):
            grp.set_order(7, [ident])
        grp.set_order(TRAIN, [ident[:40].contiguous()])
        with pytest.raises(RuntimeError, match="outside"):
            grp.step(TRAIN, 40, 20, 2, True, 0.9, 0.5)         # past n_visit: nothing is launched
        eng.set_lr(0.05)
        grp.epoch(TRAIN, 20, True, 0.9, 0.5)
        net._stream.synchronize()
        assert len(grp.results(TRAIN, 0, 20)[2]) == 2 and grp.results(TRAIN, 0, 20)[1].shape[0] == 40
        grp.close()


# ---------------------------------------------------------------------------------------------------------- grid ----
def test_sharded_grid_over_shuffle_settings(monkeypatch):
    from slnlp import grid as grid_mod
    from slnlp.grid import ShardedGridSearchCV
    ds = dataset(100, "tf_small")
    grid = {"lr": [0.05, 0.02], "iterator_train__shuffle": [False, True]}
    factory = lambda: make_net(ds, "tf_small", max_epochs=2, batch_size=20, use_graph=False, scoring=["neg_log_loss"], train_split=5)
    run = lambda **kw: ShardedGridSearchCV(factory, grid, cv=2, refit=False, device="cuda:0", **kw).fit(ds)
    res = {"one": run(lockstep=1)}
    one_at_a_time = []
    real = grid_mod.default_fit_and_score
    monkeypatch.setattr(grid_mod, "default_fit_and_score", lambda *a, **k: one_at_a_time.append(1) or real(*a, **k))
    res["lock4"] = run(lockstep=4)
    assert not one_at_a_time and res["lock4"].n_units_ < res["one"].n_units_ == 8
    monkeypatch.setattr(grid_mod, "default_fit_and_score", real)
    res["threads3"] = run(lockstep=1, fits_per_gpu=3)
    for key in ("mean_test_score", "split0_test_score", "split1_test_score"):
        for other in ("lock4", "threads3"):
            assert np.array_equal(res["one"].cv_results_[key], res[other].cv_results_[key]), (key, other)
    by = {(p["lr"], p["iterator_train__shuffle"]): s for p, s in zip(res["one"].cv_results_["params"], res["one"].cv_results_["mean_test_score"])}
    assert by[(0.05, False)] != by[(0.05, True)] and by[(0.02, False)] != by[(0.02, True)]


# -------------------------------------------------------------------------------------------------------- resume ----
@pytest.mark.parametrize("how", ["checkpoint_dir", "save_params"])
def test_resume_continues_the_order(tmp_path, how):
    """Fit 2 epochs, load the checkpoint into a fresh estimator, train the rest: epoch 3 of an uninterrupted fit.  (Dropout off:
    a checkpoint does not carry the mask stream's step counter.)"""
    ds = dataset(module="lstm")
    kw = dict(use_graph=False, module__dropout=0.0, **SHUFFLE)
    if how == "checkpoint_dir":
        kw.update(train_split=5)                                             # Checkpoint fires on valid_loss_best
    torch.manual_seed(3)
    full = make_net(ds, "lstm", max_epochs=3, **kw).fit(ds)
    torch.manual_seed(3)
    first = make_net(ds, "lstm", max_epochs=2, checkpoint_dir=str(tmp_path) if how == "checkpoint_dir" else None, **kw).fit(ds)
    if how == "save_params":
        first.save_params(str(tmp_path))
    torch.manual_seed(99)
    resumed = make_net(ds, "lstm", warm_start=True, **kw).initialize()
    assert resumed.shuffle_seed_ != full.shuffle_seed_
    resumed.load_params(str(tmp_path))
    done = len(resumed.history)                                               # the checkpoint is the best epoch's: 2 unless epoch 2 was worse
    assert resumed.shuffle_seed_ == full.shuffle_seed_ and 1 <= done <= 2 and (how != "save_params" or done == 2)
    resumed.set_params(max_epochs=3 - done)
    resumed.partial_fit(ds)
    keys = ("epoch", "train_loss", "batches", "shuffle_seed")
    assert [{k: r[k] for k in keys} for r in resumed.history[done:]] == [{k: r[k] for k in keys} for r in full.history[done:]]
    assert same_weights(resumed, full)
