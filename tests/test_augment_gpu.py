"""GPU: train-time input augmentation drawn on the device (``iterator_train__augment``).  ``slnlp_augment_rows`` against its
numpy restatement (tests/augment_ref.py) element for element; the estimator on every fit path -- eager, captured graph, GRU,
torch-stepped, lockstep, shuffled, balanced -- against fits that know nothing of the option and are fed, epoch by epoch, data
whose train-split rows were augmented ON THE HOST by the restatement; a save / load; and the option's absence."""
import numpy as np
import pytest
import torch

import augment_ref as ar
from test_loss_optim_options_gpu import make_net

pytestmark = pytest.mark.gpu

PAD, UNK = 1, 0
GRID_CAP = 2048                                       # csrc/augment.hip: blocks of four rows; beyond them the stride loop wraps
SHAPES = [(1, 1), (5, 12), (7, 64), (7, 65), (3, 130), (4 * GRID_CAP + 1, 12)]
SEEDS = (7, 0xC0FFEE1234567891)                       # the second with bits above 2^32 (the key's high word)
EPOCHS = (0, 1, 1000)
PROBS = ((0.3, 0.2), (0.0, 0.5), (0.9, 0.0), (0.0, 0.0))
GARBAGE = -(1 << 40)

_ROWS, _REF = {}, {}


def rows(shape):
    """X with garbage ids behind every row's length; lengths 0, 1, S, 2, one above S and one below 0 (both clamped), the rest
    random in [0, S]."""
    if shape not in _ROWS:
        n, S = shape
        rs = np.random.RandomState(n * 1000 + S)
        L = rs.randint(0, S + 1, size=n).astype(np.int64)
        special = (0, 1, S, min(2, S), S + 5, -3)
        L[:len(special)] = special[:n]
        if n == 1:
            L[0] = 1
        X = rs.randint(2, 3000, size=(n, S)).astype(np.int64)
        X[np.arange(S)[None, :] >= L[:, None]] = GARBAGE
        _ROWS[shape] = (X, L)
    return _ROWS[shape]


def reference(shape, probs, seed, epoch):
    key = (shape, probs, seed, epoch)
    if key not in _REF:
        X, L = rows(shape)
        _REF[key] = ar.augment_rows(X, L, PAD, UNK, probs[0], probs[1], seed, epoch)
    return _REF[key]


def rows_dropped_everywhere(shape, p_drop, seed, epoch):
    """Rows of length >= 2 whose every position drew drop: the ones the no-empty-row rule decides."""
    X, L = rows(shape)
    live, drop, _ = ar.draws(L, shape[1], p_drop, 0.0, seed, epoch)
    return np.flatnonzero((drop == live).all(axis=1) & (live.sum(axis=1) >= 2))


def seed_that_drops_a_whole_row(shape, p_drop, epoch):
    for seed in range(7, 7 + 2000):
        if len(rows_dropped_everywhere(shape, p_drop, seed, epoch)):
            return seed
    raise AssertionError(f"no seed below 2007 drops a whole row of {shape}")


# ------------------------------------------------------------------------------------------------------ the kernel ----
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_restatement(shape):
    from slnlp import ops
    X, L = rows(shape)
    Xd, Ld = torch.from_numpy(X).cuda(), torch.from_numpy(L).cuda()
    out = (torch.empty_like(Xd), torch.empty_like(Ld))
    for probs in PROBS:
        for seed in SEEDS:
            for epoch in EPOCHS:
                out[0].fill_(-77)
                out[1].fill_(-77)
                Xo, Lo = ops.augment_rows(Xd, Ld, PAD, UNK, probs[0], probs[1], seed, epoch, out=out)
                assert Xo.data_ptr() == out[0].data_ptr() and Lo.data_ptr() == out[1].data_ptr()
                want_X, want_L = reference(shape, probs, seed, epoch)
                got_X, got_L = Xo.cpu().numpy(), Lo.cpu().numpy()
                assert np.array_equal(got_L, want_L), (shape, probs, seed, epoch)
                assert np.array_equal(got_X, want_X), (shape, probs, seed, epoch)
                # the garbage behind the input's lengths reached nothing: the tail is pad
                assert (got_X[np.arange(shape[1])[None, :] >= got_L[:, None]] == PAD).all() and (got_X != GARBAGE).all()
                if probs == (0.0, 0.0):
                    assert np.array_equal(got_L, np.clip(L, 0, shape[1]))
    assert torch.equal(Xd.cpu(), torch.from_numpy(X)) and torch.equal(Ld.cpu(), torch.from_numpy(L))       # the inputs are only read
    fresh = ops.augment_rows(Xd, Ld, PAD, UNK, 0.3, 0.2, SEEDS[0], 1)                                       # out=None allocates
    assert np.array_equal(fresh[0].cpu().numpy(), reference(shape, PROBS[0], SEEDS[0], 1)[0])


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 5], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_row_that_drew_drop_everywhere_keeps_all_its_frames(shape):
    """(0.9, 0) under a seed the restatement picked so that the fixture holds a row of length >= 2 whose every position drew
    drop: the kernel must return that row whole."""
    from slnlp import ops
    X, L = rows(shape)
    epoch = 1
    seed = seed_that_drops_a_whole_row(shape, 0.9, epoch)
    whole = rows_dropped_everywhere(shape, 0.9, seed, epoch)
    assert len(whole) >= 1 and (np.clip(L[whole], 0, shape[1]) >= 2).all()            # the fixture does exercise the rule
    Xo, Lo = ops.augment_rows(torch.from_numpy(X).cuda(), torch.from_numpy(L).cuda(), PAD, UNK, 0.9, 0.0, seed, epoch)
    got_X, got_L = Xo.cpu().numpy(), Lo.cpu().numpy()
    want_X, want_L = ar.augment_rows(X, L, PAD, UNK, 0.9, 0.0, seed, epoch)
    assert np.array_equal(got_X, want_X) and np.array_equal(got_L, want_L)
    for i in whole:
        l = int(np.clip(L[i], 0, shape[1]))
        assert got_L[i] == l and np.array_equal(got_X[i, :l], X[i, :l])
    assert (got_L < np.clip(L, 0, shape[1])).any()                                    # while other rows did lose frames


def test_same_arguments_same_bits_on_any_stream():
    from slnlp import ops
    shape = SHAPES[-1]
    X, L = rows(shape)
    Xd, Ld = torch.from_numpy(X).cuda(), torch.from_numpy(L).cuda()
    a = ops.augment_rows(Xd, Ld, PAD, UNK, 0.3, 0.2, SEEDS[1], 3)
    b = ops.augment_rows(Xd, Ld, PAD, UNK, 0.3, 0.2, SEEDS[1], 3)
    torch.cuda.synchronize()
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        c = ops.augment_rows(Xd, Ld, PAD, UNK, 0.3, 0.2, SEEDS[1], 3)
    other.synchronize()
    for x in (b, c):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1], x[1])
    want = ar.augment_rows(X, L, PAD, UNK, 0.3, 0.2, SEEDS[1], 3)
    assert np.array_equal(a[0].cpu().numpy(), want[0]) and np.array_equal(a[1].cpu().numpy(), want[1])


def test_wrapper_refuses_in_place_and_bad_probabilities():
    from slnlp import ops
    X, L = rows((5, 12))
    Xd, Ld = torch.from_numpy(X).cuda(), torch.from_numpy(L).cuda()
    with pytest.raises(RuntimeError, match="not in-place"):
        ops.augment_rows(Xd, Ld, PAD, UNK, 0.3, 0.2, 7, 0, out=(Xd, torch.empty_like(Ld)))
    with pytest.raises(RuntimeError, match="not in-place"):
        ops.augment_rows(Xd, Ld, PAD, UNK, 0.3, 0.2, 7, 0, out=(torch.empty_like(Xd), Ld))
    with pytest.raises(RuntimeError, match="p_drop"):
        ops.augment_rows(Xd, Ld, PAD, UNK, 1.0, 0.2, 7, 0)
    with pytest.raises(RuntimeError, match="epoch"):
        ops.augment_rows(Xd, Ld, PAD, UNK, 0.3, 0.2, 7, -1)


# --------------------------------------------------------------------------------------------------- the estimator ----
AUG = {"frame_drop": 0.3, "token_mask": 0.2}
NOT_COMPARED = ("dur", "augment_seed", "valid_loss_best")      # (a one-epoch partial_fit starts its best-so-far afresh)


def dataset():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(100, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


def strip(history, drop=NOT_COMPARED):
    return [{k: v for k, v in row.items() if k not in drop} for row in history]


def same_weights(a, b):
    sa, sb = a.module_.state_dict(), b.module_.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


def host_augmented(ds, idx_tr, setting, seed, epoch):
    """``ds`` with its TRAIN-SPLIT rows augmented by the restatement -- the counter's row is the index inside the train split --
    and every other row untouched."""
    from slnlp.data import TokenDataset
    X, L = ds.ids.copy(), ds.lengths.copy()
    X[idx_tr], L[idx_tr] = ar.augment_rows(ds.ids[idx_tr], ds.lengths[idx_tr], PAD, UNK, setting.get("frame_drop", 0.0),
                                           setting.get("token_mask", 0.0), seed, epoch)
    return TokenDataset(X, L, ds.y, ds.vocab_X, ds.vocab_y)


def fit_pair(ds, module, setting, torch_seed, epochs=2, **kw):
    """(the fit with the option, the fit without it fed host-augmented data one epoch at a time), both from ``torch_seed``."""
    torch.manual_seed(torch_seed)
    net = make_net(ds, module, max_epochs=epochs, scoring=["accuracy", "neg_log_loss"], iterator_train__augment=setting, **kw).fit(ds)
    assert isinstance(net.augment_seed_, int) and all(row["augment_seed"] == net.augment_seed_ for row in net.history)
    idx_tr, idx_va = net._train_split(ds)
    torch.manual_seed(torch_seed)
    ref = make_net(ds, module, max_epochs=1, scoring=["accuracy", "neg_log_loss"], **kw).initialize()
    assert ref.augment_seed_ is None
    for epoch in range(epochs):
        fed = host_augmented(ds, idx_tr, setting, net.augment_seed_, epoch)
        if idx_va is not None:
            assert np.array_equal(fed.ids[idx_va], ds.ids[idx_va]) and np.array_equal(fed.lengths[idx_va], ds.lengths[idx_va])
        assert not np.array_equal(fed.ids[idx_tr], ds.ids[idx_tr])
        ref.partial_fit(fed)
    assert all("augment_seed" not in row for row in ref.history)
    return net, ref


def assert_same_fit(net, ref, epochs=2):
    assert len(net.history) == len(ref.history) == epochs
    for a, b in zip(net.history, ref.history):
        for key in ("train_loss", "valid_loss", "train_accuracy", "train_neg_log_loss", "valid_accuracy", "valid_neg_log_loss"):
            assert (key in a) == (key in b) and a.get(key) == b.get(key), (key, a.get(key), b.get(key))
    assert strip(net.history) == strip(ref.history)              # the batch losses and sizes too
    assert same_weights(net, ref)


PATHS = {"tf_eager": ("tf", dict(use_graph=False)),
         "tf_graph": ("tf", dict(use_graph=True)),
         "gru": ("gru", dict(use_graph=False)),                   # the lengths drive the packing
         "torch_stepped": ("tf", dict(optimizer="torch.optim.RMSprop", lr=1e-3))}


@pytest.mark.parametrize("path", list(PATHS))
def test_an_augmented_fit_is_one_epoch_fits_on_host_augmented_data(path):
    module, kw = PATHS[path]
    ds = dataset()
    net, ref = fit_pair(ds, module, AUG, 21, **kw)
    assert net._fused == (path != "torch_stepped") and "valid_loss" in net.history[0]
    assert_same_fit(net, ref)
    # and the option did something: the same fit without it trains on other inputs
    torch.manual_seed(21)
    plain = make_net(ds, module, max_epochs=2, scoring=["accuracy", "neg_log_loss"], **kw).fit(ds)
    assert [r["train_loss"] for r in plain.history] != [r["train_loss"] for r in net.history]


@pytest.mark.parametrize("module", ["tf", "gru"])
def test_lockstep_group_of_differently_augmented_fits_equals_solo_fits(module):
    from slnlp.lockstep import fit_lockstep
    ds = dataset()
    settings = [dict(iterator_train__augment=AUG), dict(iterator_train__augment={"token_mask": 0.4}, lr=0.02), dict()]

    def build():
        nets = []
        for i, kw in enumerate(settings):
            torch.manual_seed(40 + i)
            nets.append(make_net(ds, module, use_graph=False, max_epochs=2, scoring=["neg_log_loss", "accuracy"], **kw).initialize())
        return nets
    solo = build()
    for n in solo:
        n.partial_fit(ds)
    lock = build()
    fit_lockstep(lock, [ds] * 3)
    for a, b in zip(solo, lock):
        assert a._fused and a.augment_seed_ == b.augment_seed_
        assert strip(a.history, ("dur",)) == strip(b.history, ("dur",)) and same_weights(a, b)
    assert isinstance(lock[0].augment_seed_, int) and isinstance(lock[1].augment_seed_, int) and lock[2].augment_seed_ is None
    assert "augment_seed" in lock[0].history[0] and "augment_seed" not in lock[2].history[0] and len(lock[0].history) == 2
    # the group's first member is the host-augmented fit of the solo test, not merely equal to its own solo run
    idx_tr, _ = lock[0]._train_split(ds)
    torch.manual_seed(40)
    ref = make_net(ds, module, use_graph=False, max_epochs=1, scoring=["neg_log_loss", "accuracy"]).initialize()
    for epoch in range(2):
        ref.partial_fit(host_augmented(ds, idx_tr, AUG, lock[0].augment_seed_, epoch))
    assert_same_fit(lock[0], ref)


@pytest.mark.parametrize("other", ["shuffle", "balance"])
def test_beside_shuffling_or_balancing_the_rows_are_host_augmented_rows_in_the_same_order(other):
    """The reference shuffles / balances too (same seed: the first draw after the weights under one torch seed) and knows
    nothing of augmentation: the order picks rows, the draw is per dataset row."""
    ds = dataset()
    kw = {f"iterator_train__{other}": True, "use_graph": False}
    net, ref = fit_pair(ds, "gru", AUG, 33, **kw)
    if other == "shuffle":
        assert net.shuffle_seed_ is not None and net.shuffle_seed_ == ref.shuffle_seed_
    else:
        assert net.balance_seed_ is not None and net.balance_seed_ == ref.balance_seed_
    assert net.augment_seed_ not in (net.shuffle_seed_, net.balance_seed_)
    assert_same_fit(net, ref)


def test_resumed_fit_continues_the_draws(tmp_path):
    ds = dataset()
    torch.manual_seed(9)
    whole = make_net(ds, "gru", use_graph=False, max_epochs=2, iterator_train__augment=AUG).fit(ds)
    torch.manual_seed(9)
    first = make_net(ds, "gru", use_graph=False, max_epochs=1, iterator_train__augment=AUG).fit(ds)
    first.save_params(str(tmp_path))
    torch.manual_seed(1234)                               # another seed: everything the resumed fit needs is in the checkpoint
    second = make_net(ds, "gru", use_graph=False, max_epochs=1, iterator_train__augment=AUG).initialize()
    assert second.augment_seed_ != first.augment_seed_
    second.load_params(str(tmp_path))
    assert second.augment_seed_ == first.augment_seed_ == whole.augment_seed_
    second.partial_fit(ds)
    assert len(second.history) == 2 and all(row["augment_seed"] == whole.augment_seed_ for row in second.history)
    drop = ("dur", "valid_loss_best")
    assert strip(second.history, drop) == strip(whole.history, drop) and same_weights(second, whole)


def test_without_the_option_nothing_changes():
    ds = dataset()
    fits = []
    for kw in (dict(), dict(iterator_train__augment=None), dict(iterator_train__augment=False)):
        torch.manual_seed(17)
        fits.append(make_net(ds, "tf", max_epochs=2, **kw).fit(ds))
    for n in fits:
        assert n.augment_seed_ is None and all("augment_seed" not in row for row in n.history)
        assert strip(n.history, ("dur",)) == strip(fits[0].history, ("dur",)) and same_weights(n, fits[0])

    def second_after(**kw):
        """The initial weights of an estimator initialised SECOND under one torch seed, behind one with ``kw``."""
        torch.manual_seed(5)
        make_net(ds, "tf", **kw).initialize()
        return make_net(ds, "tf").initialize()
    absent, off, on = second_after(), second_after(iterator_train__augment=False), second_after(iterator_train__augment=AUG)
    assert same_weights(absent, off)                      # without the option, initialize() consumes what it always did
    assert not same_weights(absent, on)                   # (with it, one draw more: the comparison does see the generator)
