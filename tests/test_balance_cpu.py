"""CPU: the class-balanced epoch draw (``iterator_train__balance``) -- invariants of its numpy restatement (tests/balance_ref.py,
which tests/test_balance_gpu.py holds the kernel to), the option's validation, the RNG consumption of a configuration without
it, and the C ABI's new symbols."""
import os
import re

import numpy as np
import pytest
import torch

import balance_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 2, 5, 9, 20, 63)
SYMBOLS = ("slnlp_balance_plan_create", "slnlp_balance_plan_rows", "slnlp_balance_plan_destroy", "slnlp_balanced_order")


def labels(counts, seed=0):
    y = np.repeat(np.arange(len(counts)), counts)
    return np.random.RandomState(seed).permutation(y).astype(np.int64)


@pytest.mark.parametrize("counts", [COUNTS, (17,)], ids=["six_classes", "one_class"])
def test_restatement_invariants(counts):
    y = labels(counts)
    classes, under, over = br.targets(y)
    assert classes == list(range(len(counts)))
    if counts == COUNTS:
        # sampling_targets by hand: u = 100 / 6; smooth(v) = round(u + ln v)
        assert under == [1, 2, 5, 9, 20, 21] and over == [17, 17, 18, 19, 20, 21]
    seed = 0x1234567890ABCDEF
    orders = []
    for epoch in range(5):
        order, y_visit = br.balanced_order(y, seed, epoch)
        assert order.dtype == np.int64 and order.shape == (sum(over),) == (br.balanced_rows(y),)
        assert order.min() >= 0 and order.max() < len(y) and np.array_equal(y_visit, y[order])
        assert np.bincount(y_visit, minlength=len(counts)).tolist() == over
        for c, u in zip(classes, under):
            assert len(set(order[y_visit == c].tolist())) == u          # the rows visited are the u_c kept ones, all distinct rows
        again, _ = br.balanced_order(y, seed, epoch)
        assert np.array_equal(order, again)
        orders.append(order)
    for a in range(5):
        for b in range(a + 1, 5):
            assert not np.array_equal(orders[a], orders[b])
    assert not np.array_equal(orders[0], br.balanced_order(y, seed + 1, 0)[0])


def test_every_row_of_the_large_class_is_visited_within_200_epochs():
    """The under-sample is redrawn every epoch: 21 of the class's 63 rows are kept per epoch, so a row stays unseen through 200
    epochs with probability (2 / 3) ** 200 ~ 6e-36 -- the restatement alone meets the 200 epochs the check was given."""
    y = labels(COUNTS)
    big = set(np.flatnonzero(y == 5).tolist())
    seen = set()
    for epoch in range(200):
        order, y_visit = br.balanced_order(y, 99, epoch)
        seen |= set(order[y_visit == 5].tolist())
    assert seen == big


def test_epoch_length_helper_agrees_with_the_restatement():
    from slnlp import sampler
    for counts in (COUNTS, (17,), (1, 6), (3, 3, 3)):
        y = labels(counts)
        assert sampler.balanced_rows(y) == br.balanced_rows(y)
    assert sampler.HONOURED == ("shuffle", "drop_last") and sampler.BALANCE == "balance"


def make_net(**kw):
    from slnlp.net import NeuralNetClassifier
    return NeuralNetClassifier(module="model.Transformer", **kw)


def test_option_values():
    assert make_net()._iterator_train_balance() is False
    assert make_net(iterator_train__balance=False)._iterator_train_balance() is False
    assert make_net(iterator_train__balance=True)._iterator_train_balance() is True
    assert make_net(iterator_train__balance=True, iterator_train__shuffle=True)._iterator_train() == (True, False)   # still a two-tuple
    for bad in ("yes", 1, None):
        net = make_net(iterator_train__balance=bad)
        with pytest.raises(ValueError, match="iterator_train__balance"):
            net._iterator_train_balance()
        with pytest.raises(ValueError, match="iterator_train__balance"):
            net.initialize()                                              # raised before anything is built or drawn


def test_rng_consumption_without_the_option_is_unchanged():
    def after(**kw):
        net = make_net(**kw)
        torch.manual_seed(123)
        net._draw_iterator_seeds(net._iterator_train()[0], net._iterator_train_balance())
        return net, float(torch.rand(1))
    torch.manual_seed(123)
    untouched = float(torch.rand(1))
    absent, r_absent = after()
    off, r_off = after(iterator_train__balance=False)
    on, r_on = after(iterator_train__balance=True)
    assert r_absent == r_off == untouched and absent.balance_seed_ is None and off.balance_seed_ is None
    assert r_on != untouched and isinstance(on.balance_seed_, int) and on.shuffle_seed_ is None
    # with shuffling on as well the shuffle seed is the first draw, as it was
    both, _ = after(iterator_train__shuffle=True, iterator_train__balance=True)
    only, _ = after(iterator_train__shuffle=True)
    assert both.shuffle_seed_ == only.shuffle_seed_ and both.balance_seed_ not in (None, both.shuffle_seed_)


def test_abi_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slnlp.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} not declared in slnlp.h"
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    # argument errors are codes with a message and need no GPU: they are found before anything touches the device
    import ctypes as C
    out = C.c_void_p()
    y = np.array([0, 1, 2], dtype=np.int64)
    assert lib.slnlp_balance_plan_create(y.ctypes.data, 3, 2, None, C.byref(out)) == 1 and not out.value      # label == n_classes
    assert b"label" in lib.slnlp_last_error()
    assert lib.slnlp_balance_plan_create(None, 3, 3, None, C.byref(out)) == 1
    assert lib.slnlp_balance_plan_create(y.ctypes.data, 0, 3, None, C.byref(out)) == 1
    assert lib.slnlp_balance_plan_create(y.ctypes.data, 3, 3, None, None) == 1
    assert lib.slnlp_balanced_order(None, None, 0, 0, None, None, None) == 1
    assert lib.slnlp_balance_plan_rows(None) == -1
