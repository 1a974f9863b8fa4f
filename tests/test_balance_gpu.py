"""GPU: class-balanced train epochs drawn on the device (``iterator_train__balance``).  ``slnlp_balanced_order`` against its
numpy restatement (tests/balance_ref.py) element for element; the estimator on every fit path -- eager, captured graph,
torch-stepped, lockstep -- against one-epoch fits on data resampled ON THE HOST by the restatement, against each other, and
through a save / load; and the option's absence against the code path as it was."""
import ctypes as C

import numpy as np
import pytest
import torch

import balance_ref as br
from test_loss_optim_options_gpu import make_net

pytestmark = pytest.mark.gpu

SEEDS = (7, 0xC0FFEE1234567891)                       # the second with bits above 2^32 (the key's high word)
EPOCHS = (0, 1, 1000)


def labels(counts, seed=0):
    y = np.repeat(np.arange(len(counts)), counts)
    return np.random.RandomState(seed).permutation(y).astype(np.int64)


def big_counts():
    """37 classes, 4099 rows, the largest of 600: its rows span three workgroups of the ranking launch, the shuffle ~67."""
    c = [600, 300, 257, 1, 2] + [45 + 3 * k for k in range(32)]
    c[-1] += 4099 - sum(c)
    assert len(c) == 37 and sum(c) == 4099 and min(c) >= 1 and max(c) > 256
    return tuple(c)


CASES = {"n100": (1, 2, 5, 9, 20, 63), "n7": (1, 6), "one_class": (17,), "n4099": big_counts()}
_REF = {}


def reference(case, seed, epoch):
    key = (case, seed, epoch)
    if key not in _REF:
        _REF[key] = br.balanced_order(labels(CASES[case]), seed, epoch)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------ the kernel ----
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_equals_the_restatement(case):
    from slnlp import ops
    y = labels(CASES[case])
    yd = torch.from_numpy(y).cuda()
    plan = ops.BalancePlan(y, len(CASES[case]) + 2)      # (classes nobody has take no part)
    assert plan.rows == br.balanced_rows(y)
    for seed in SEEDS:
        for epoch in EPOCHS:
            order, y_visit = plan.order(yd, seed, epoch)
            want, y_want = reference(case, seed, epoch)
            assert np.array_equal(order.cpu().numpy(), want), (case, seed, epoch)
            assert np.array_equal(y_visit.cpu().numpy(), y_want)
    only, none = plan.order(yd, SEEDS[0], 1, want_labels=False)          # y_out NULL: the order alone
    assert none is None and np.array_equal(only.cpu().numpy(), reference(case, SEEDS[0], 1)[0])


def test_same_arguments_same_bits_on_any_stream():
    from slnlp import ops
    y = labels(CASES["n4099"])
    yd = torch.from_numpy(y).cuda()
    plan = ops.BalancePlan(y, 37)
    a = plan.order(yd, SEEDS[1], 3)
    b = plan.order(yd, SEEDS[1], 3)
    torch.cuda.synchronize()
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        c = plan.order(yd, SEEDS[1], 3)
    other.synchronize()
    for x in (b, c):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1], x[1])
    assert np.array_equal(a[0].cpu().numpy(), br.balanced_order(y, SEEDS[1], 3)[0])


def test_argument_errors_are_codes():
    from slnlp._lib import load, ptr
    lib = load()
    st = torch.cuda.current_stream().cuda_stream
    y = labels((1, 6))
    out = C.c_void_p()
    bad = y.copy()
    bad[3] = 2
    assert lib.slnlp_balance_plan_create(bad.ctypes.data, 7, 2, st, C.byref(out)) == 1 and not out.value       # a label == n_classes
    assert b"label" in lib.slnlp_last_error()
    assert lib.slnlp_balance_plan_create(y.ctypes.data, 7, 2, st, C.byref(out)) == 0 and out.value
    yd = torch.from_numpy(y).cuda()
    o = torch.empty(int(lib.slnlp_balance_plan_rows(out)), dtype=torch.int64, device="cuda")
    assert lib.slnlp_balanced_order(out, ptr(yd), 1, 0, None, ptr(o), st) == 1                                 # null order_out
    assert b"order_out" in lib.slnlp_last_error()
    assert lib.slnlp_balanced_order(out, None, 1, 0, ptr(o), ptr(o), st) == 1                                  # y_out without labels
    assert lib.slnlp_balanced_order(out, ptr(yd), 1, -1, ptr(o), None, st) == 1                                # epoch < 0
    assert lib.slnlp_balanced_order(out, ptr(yd), 1, 0, ptr(o), None, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), br.balanced_order(y, 1, 0)[0])
    lib.slnlp_balance_plan_destroy(out)


# --------------------------------------------------------------------------------------------------- the estimator ----
BALANCE = dict(iterator_train__balance=True)
COUNTS = (5, 6, 9, 15, 25, 40)                        # 100 rows, labels 2 .. 7 (0 / 1 are <unk> / <pad>)


def dataset(counts=COUNTS):
    """Rows of the synthetic dataset picked so that label 2 + c has counts[c] rows, in a fixed shuffled order."""
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(400, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)
    idx = np.concatenate([np.flatnonzero(ds.y == 2 + c)[:k] for c, k in enumerate(counts)])
    assert len(idx) == sum(counts)
    return ds[np.random.RandomState(3).permutation(idx)]


def strip(history):
    return [{k: v for k, v in row.items() if k != "dur"} for row in history]


def same_weights(a, b):
    sa, sb = a.module_.state_dict(), b.module_.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


def train_sizes(net):
    return [[b["train_batch_size"] for b in row["batches"] if "train_batch_size" in b] for row in net.history]


def batch_losses(net, key="train_loss"):
    return [[b[key] for b in row["batches"] if key in b] for row in net.history]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("module", ["tf", "lstm"])
def test_a_balanced_fit_is_one_epoch_fits_on_host_resampled_data(module, graph):
    """The definition: the fit's own train split, resampled per epoch by the restatement ON THE HOST and trained for one epoch
    by an estimator that knows nothing of balancing, gives the same batch losses and weights, bit for bit.  The valid pass
    sees the untouched valid split: its sizes, and its accuracy against a fresh prediction on exactly those rows."""
    ds = dataset()
    torch.manual_seed(21)
    net = make_net(ds, module, use_graph=graph, scoring=["accuracy"], **BALANCE).fit(ds)
    assert net._fused and isinstance(net.balance_seed_, int) and net.shuffle_seed_ is None
    assert all(row["balance_seed"] == net.balance_seed_ and "shuffle_seed" not in row for row in net.history)
    idx_tr, idx_va = net._train_split(ds)
    tr, va = ds[idx_tr], ds[idx_va]
    n_bal = br.balanced_rows(tr.y)
    assert n_bal > len(tr)                                # (small classes are visited more often than they have rows)
    assert train_sizes(net) == [[20] * (n_bal // 20) + ([n_bal % 20] if n_bal % 20 else [])] * 3
    assert [sum(b["valid_batch_size"] for b in row["batches"] if "valid_batch_size" in b) for row in net.history] == [len(va)] * 3
    torch.manual_seed(21)
    ref = make_net(ds, module, use_graph=graph, max_epochs=1, train_split=None).initialize()
    for epoch in range(3):
        order, _ = br.balanced_order(tr.y, net.balance_seed_, epoch)
        ref.partial_fit(tr[order])
    assert all("balance_seed" not in row for row in ref.history)
    assert batch_losses(net) == batch_losses(ref) and same_weights(net, ref)
    assert net.history[-1]["valid_accuracy"] == float((net.predict(va) == va.y).mean())
    hist = np.bincount(tr.y[br.balanced_order(tr.y, net.balance_seed_, 0)[0]], minlength=8)[2:]
    skew = np.bincount(tr.y, minlength=8)[2:]
    assert hist.max() - hist.min() <= 4 < skew.max() - skew.min()          # balanced visits from skewed counts


@pytest.mark.parametrize("module", ["tf", "lstm"])
def test_eager_graph_and_torch_stepped_fits_agree(module):
    ds = dataset()
    nets = {}
    for path in ("eager", "graph", "torch"):
        torch.manual_seed(11)
        net = make_net(ds, module, use_graph=(path == "graph"), **BALANCE).initialize()
        assert net._fused
        if path == "torch":                               # force the stock-optimizer path around the autograd bridge
            net._fused, net._fused_kind = False, None
            net.optimizer_ = net._opt_cls(net.module_.parameters(), lr=net.lr, **net._opt_kwargs)
        nets[path] = net.partial_fit(ds)
    assert len({n.balance_seed_ for n in nets.values()}) == 1
    assert strip(nets["eager"].history) == strip(nets["graph"].history) and same_weights(nets["eager"], nets["graph"])
    assert train_sizes(nets["torch"]) == train_sizes(nets["eager"])
    for key in ("train_loss", "valid_loss"):
        a, b = [h[key] for h in nets["eager"].history], [h[key] for h in nets["torch"].history]
        print(module, key, max(abs(x - y) / abs(y) for x, y in zip(a, b)))
        assert np.allclose(a, b, rtol=1e-4), (key, a, b)


def test_drop_last_visits_the_full_batches_of_the_balanced_epoch():
    ds = dataset()
    torch.manual_seed(5)
    net = make_net(ds, "gru", use_graph=False, iterator_train__drop_last=True, iterator_train__shuffle=True, **BALANCE).fit(ds)
    n_bal = br.balanced_rows(ds.y[net._train_split(ds)[0]])
    assert n_bal % 20 and train_sizes(net) == [[20] * (n_bal // 20)] * 3
    torch.manual_seed(5)
    plain = make_net(ds, "gru", use_graph=False, iterator_train__drop_last=True, **BALANCE).initialize()
    # the draw already permutes: shuffle beside it only draws its (unused) seed -- after the weights, in front of the balance seed
    assert net.shuffle_seed_ is not None and plain.shuffle_seed_ is None and plain.balance_seed_ == net.shuffle_seed_
    plain.balance_seed_ = net.balance_seed_
    plain.partial_fit(ds)
    assert all("shuffle_seed" not in row for row in net.history)
    assert batch_losses(net) == batch_losses(plain) and same_weights(net, plain)


@pytest.mark.parametrize("module", ["tf", "lstm"])
def test_lockstep_group_of_balanced_fits_equals_solo_fits(module):
    from slnlp.lockstep import fit_lockstep
    ds = dataset()
    settings = [dict(), dict(lr=0.02), dict()]

    def build():
        nets = []
        for i, kw in enumerate(settings):
            torch.manual_seed(40 + i)
            nets.append(make_net(ds, module, use_graph=False, scoring=["neg_log_loss", "accuracy"], **BALANCE, **kw).initialize())
        return nets
    solo = build()
    for n in solo:
        n.partial_fit(ds)
    lock = build()
    fit_lockstep(lock, [ds] * 3)
    for a, b in zip(solo, lock):
        assert a._fused and a.balance_seed_ == b.balance_seed_
        assert strip(a.history) == strip(b.history) and same_weights(a, b)
    assert len({n.balance_seed_ for n in lock}) == 3 and len(lock[0].history) == 3
    n_bal = br.balanced_rows(ds.y[lock[0]._train_split(ds)[0]])
    assert [sum(s) for s in train_sizes(lock[0])] == [n_bal] * 3


def test_resumed_fit_continues_the_draws(tmp_path):
    ds = dataset()
    torch.manual_seed(9)
    whole = make_net(ds, "lstm", use_graph=False, max_epochs=4, **BALANCE).fit(ds)
    torch.manual_seed(9)
    first = make_net(ds, "lstm", use_graph=False, max_epochs=2, **BALANCE).fit(ds)
    first.save_params(str(tmp_path))
    torch.manual_seed(1234)                               # another seed: everything the resumed fit needs is in the checkpoint
    second = make_net(ds, "lstm", use_graph=False, max_epochs=2, **BALANCE).initialize()
    assert second.balance_seed_ != first.balance_seed_
    second.load_params(str(tmp_path))
    assert second.balance_seed_ == first.balance_seed_
    second.partial_fit(ds)
    assert len(second.history) == 4 and all(row["balance_seed"] == whole.balance_seed_ for row in second.history)
    assert strip(second.history) == strip(whole.history) and same_weights(second, whole)


@pytest.mark.parametrize("module", ["tf", "lstm"])
def test_without_the_option_nothing_changes(module):
    ds = dataset()
    fits = []
    for kw in (dict(), dict(iterator_train__balance=False)):
        torch.manual_seed(17)
        fits.append(make_net(ds, module, **kw).fit(ds))
    absent, off = fits
    assert strip(absent.history) == strip(off.history) and same_weights(absent, off)
    assert all("balance_seed" not in row for n in fits for row in n.history)
    assert absent.balance_seed_ is None and off.balance_seed_ is None
    n_tr = len(absent._train_split(ds)[0])
    assert [sum(s) for s in train_sizes(absent)] == [n_tr] * 3
