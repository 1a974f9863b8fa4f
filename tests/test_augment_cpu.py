"""CPU: train-time input augmentation (``iterator_train__augment``) -- invariants of the draw's numpy restatement
(tests/augment_ref.py, which tests/test_augment_gpu.py holds the kernel to), the option's validation, the RNG consumption of a
configuration without it, the C entry's argument checks (no GPU needed: they run before any launch) and the grid's grouping."""
import numpy as np
import pytest
import torch

import augment_ref as ar
from threefry_ref import threshold

PAD, UNK = 1, 0


def random_rows(n, S, seed, vocab=50):
    """Ids in [2, vocab) -- never pad or unk -- with garbage (negative ids) behind every row's length; lengths cover 0, 1 and S."""
    rs = np.random.RandomState(seed)
    L = rs.randint(0, S + 1, size=n).astype(np.int64)
    L[:3] = (0, 1, S)[:min(3, n)]
    X = rs.randint(2, vocab, size=(n, S)).astype(np.int64)
    X[np.arange(S)[None, :] >= L[:, None]] = -12345
    return X, L


def is_subsequence_with_unk(out, src):
    """Whether ``out`` is ``src`` with some elements deleted and some of the rest replaced by UNK, order kept -- greedy matching
    is exact because UNK never occurs in ``src``: an UNK consumes one source element, any other token the next equal one."""
    j = 0
    for tok in out:
        if tok == UNK:
            j += 1
        else:
            while j < len(src) and src[j] != tok:
                j += 1
            j += 1
        if j > len(src):
            return False
    return True


@pytest.mark.parametrize("p_drop,p_mask", [(0.3, 0.2), (0.0, 0.5), (0.9, 0.0), (0.97, 0.97)])
def test_restatement_invariants(p_drop, p_mask):
    n, S = 300, 23
    X, L = random_rows(n, S, seed=1)
    for seed, epoch in ((7, 0), (0xC0FFEE1234567891, 1000)):
        Xo, Lo = ar.augment_rows(X, L, PAD, UNK, p_drop, p_mask, seed, epoch)
        assert Xo.dtype == np.int64 and Xo.shape == X.shape and Lo.dtype == np.int64 and Lo.shape == L.shape
        assert ((Lo >= 1) == (L >= 1)).all() and (Lo <= L).all()                # a row never loses all of its frames
        for i in range(n):
            assert (Xo[i, Lo[i]:] == PAD).all()                                 # the tail, whatever lay behind the input's length
            assert is_subsequence_with_unk(Xo[i, :Lo[i]].tolist(), X[i, :L[i]].tolist()), i
            if p_mask == 0.0:
                assert UNK not in Xo[i, :Lo[i]]
        if p_drop == 0.0:
            assert np.array_equal(Lo, L)
        again = ar.augment_rows(X, L, PAD, UNK, p_drop, p_mask, seed, epoch)
        assert np.array_equal(Xo, again[0]) and np.array_equal(Lo, again[1])
        other = ar.augment_rows(X, L, PAD, UNK, p_drop, p_mask, seed, epoch + 1)
        assert not np.array_equal(Xo, other[0])
    if p_drop >= 0.9:                                       # the rule is exercised: some row of length >= 2 drew drop everywhere
        live, drop, _ = ar.draws(L, S, p_drop, p_mask, 7, 0)
        assert ((drop == live).all(axis=1) & (L >= 2)).any()


def test_zero_probabilities_are_the_identity_on_the_live_positions():
    X, L = random_rows(200, 17, seed=2)
    Xo, Lo = ar.augment_rows(X, L, PAD, UNK, 0.0, 0.0, 99, 3)
    assert np.array_equal(Lo, L)
    live = np.arange(17)[None, :] < L[:, None]
    assert np.array_equal(Xo[live], X[live]) and (Xo[~live] == PAD).all()


def test_rows_parameter_is_the_counter_and_a_row_does_not_depend_on_its_neighbours():
    X, L = random_rows(40, 12, seed=3)
    whole = ar.augment_rows(X, L, PAD, UNK, 0.3, 0.2, 5, 2)
    idx = np.array([31, 4, 17])
    part = ar.augment_rows(X[idx], L[idx], PAD, UNK, 0.3, 0.2, 5, 2, rows=idx)
    assert np.array_equal(part[0], whole[0][idx]) and np.array_equal(part[1], whole[1][idx])


@pytest.mark.parametrize("p_drop,p_mask", [(0.3, 0.2), (0.05, 0.5)])
def test_draw_frequencies_are_the_thresholds(p_drop, p_mask):
    """2 * 10^5 positions; each frequency within 4 binomial standard deviations of thr16 / 65536; drop and mask read disjoint
    halves of the word, so their joint frequency is the product's, within the same bound."""
    n, S = 4000, 50
    L = np.full(n, S, dtype=np.int64)
    live, drop, mask = ar.draws(L, S, p_drop, p_mask, 0x1234567890ABCDEF, 4)
    N = n * S
    assert live.all() and N == 200000
    for got, p in ((drop.mean(), threshold(p_drop) / 65536), (mask.mean(), threshold(p_mask) / 65536),
                   ((drop & mask).mean(), threshold(p_drop) * threshold(p_mask) / 65536 ** 2)):
        assert abs(got - p) <= 4 * np.sqrt(p * (1 - p) / N), (got, p)


# ------------------------------------------------------------------------------------------------------ the option ----
def make_net(**kw):
    from slnlp.net import NeuralNetClassifier
    return NeuralNetClassifier(module="model.Transformer", **kw)


def test_option_values_and_defaults():
    from slnlp import sampler
    assert sampler.AUGMENT == "augment" and sampler.AUGMENT_KEYS == ("frame_drop", "token_mask")
    for off in (None, False):
        assert sampler.augment_options(off) is None
        assert make_net(iterator_train__augment=off)._iterator_train_augment() is None
    assert make_net()._iterator_train_augment() is None
    assert sampler.augment_options({}) == {"frame_drop": 0.0, "token_mask": 0.0}
    assert sampler.augment_options({"frame_drop": 0.25}) == {"frame_drop": 0.25, "token_mask": 0.0}
    assert sampler.augment_options({"token_mask": np.float32(0.5)}) == {"frame_drop": 0.0, "token_mask": 0.5}
    assert make_net(iterator_train__augment={"frame_drop": 0, "token_mask": 0.1})._iterator_train_augment() == \
        {"frame_drop": 0.0, "token_mask": 0.1}
    bad = [True, "frame_drop", 0.3, [("frame_drop", 0.3)],                                        # not a dict
           {"frame_dropout": 0.1}, {"frame_drop": 0.1, "p": 0.2}, {1: 0.2},                        # unknown keys
           {"frame_drop": 1.0}, {"frame_drop": -0.01}, {"token_mask": 1.5}, {"token_mask": float("nan")},
           {"token_mask": 0.99999999},                                                             # 1.0 as the float32 the library takes
           {"frame_drop": "0.1"}, {"frame_drop": None}, {"token_mask": True}, {"frame_drop": 0.1 + 0j}]
    for setting in bad:
        with pytest.raises(ValueError, match="iterator_train__augment"):
            sampler.augment_options(setting)
        net = make_net(iterator_train__augment=setting)
        with pytest.raises(ValueError, match="iterator_train__augment"):
            net.initialize()                                                  # raised before anything is built or drawn
    assert make_net(iterator_train__augment={"frame_drop": 0.1}, iterator_train__shuffle=True)._iterator_train() == (True, False)


def test_pad_and_unk_come_from_the_source_vocabulary():
    from model.util import Vocab
    assert make_net(module__src_vocab=Vocab(20))._augment_ids() == (1, 0)
    assert make_net(module__src_vocab=Vocab(["<pad>", "a", "<unk>", "b"]))._augment_ids() == (1, 0)
    with pytest.raises(ValueError, match="source vocabulary"):
        make_net(iterator_train__augment={"frame_drop": 0.1}).initialize()


def test_rng_consumption_without_the_option_is_unchanged():
    def after(**kw):
        net = make_net(**kw)
        torch.manual_seed(123)
        net._draw_iterator_seeds(net._iterator_train()[0], net._iterator_train_balance(), net._iterator_train_augment() is not None)
        return net, float(torch.rand(1))
    torch.manual_seed(123)
    untouched = float(torch.rand(1))
    for kw in (dict(), dict(iterator_train__augment=None), dict(iterator_train__augment=False)):
        net, r = after(**kw)
        assert r == untouched and net.augment_seed_ is None
    on, r_on = after(iterator_train__augment={"token_mask": 0.1})
    assert r_on != untouched and isinstance(on.augment_seed_, int) and on.shuffle_seed_ is None and on.balance_seed_ is None
    # beside the other two the augment seed is the last draw: theirs stay what they were
    three, _ = after(iterator_train__shuffle=True, iterator_train__balance=True, iterator_train__augment={"frame_drop": 0.1})
    two, _ = after(iterator_train__shuffle=True, iterator_train__balance=True)
    assert (three.shuffle_seed_, three.balance_seed_) == (two.shuffle_seed_, two.balance_seed_)
    assert three.augment_seed_ not in (None, three.shuffle_seed_, three.balance_seed_)
    # the two-argument call of before still stands
    net = make_net()
    net._draw_iterator_seeds(False, False)
    assert net.augment_seed_ is None


# --------------------------------------------------------------------------------------------------- the C entry ----
def test_argument_errors_are_codes_with_a_message():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    lib = _lib.load()
    assert "slnlp_augment_rows" in _lib.SIGNATURES
    n, S = 4, 6
    X, L = np.zeros((n, S), np.int64), np.zeros(n, np.int64)
    Xo, Lo = np.zeros((n, S), np.int64), np.zeros(n, np.int64)
    p = lambda a: a.ctypes.data
    good = dict(X=p(X), L=p(L), n=n, S=S, p_drop=0.3, p_mask=0.2, epoch=0, X_out=p(Xo), L_out=p(Lo))

    def refused(word, **change):
        a = dict(good, **change)
        rc = lib.slnlp_augment_rows(a["X"], a["L"], a["n"], a["S"], PAD, UNK, a["p_drop"], a["p_mask"], 7, a["epoch"], a["X_out"],
                                    a["L_out"], None)
        msg = lib.slnlp_last_error()
        assert rc == 1, (change, rc)
        assert b"augment_rows" in msg and word in msg, (change, msg)

    for name in ("X", "L", "X_out", "L_out"):
        refused(b"null", **{name: None})
    refused(b"n=0", n=0)
    refused(b"n=-2", n=-2)
    refused(b"n=2147483648", n=1 << 31)                     # beyond an int32 row index
    refused(b"S=0", S=0)
    refused(b"S=-1", S=-1)
    refused(b"epoch -1", epoch=-1)
    refused(b"epoch 4294967296", epoch=1 << 32)             # the counter word is 32 bits
    refused(b"p_drop=1", p_drop=1.0)
    refused(b"p_drop=-0.5", p_drop=-0.5)
    refused(b"p_drop=nan", p_drop=float("nan"))
    refused(b"p_mask=1.5", p_mask=1.5)
    refused(b"p_mask=-1", p_mask=-1.0)
    refused(b"not in-place", X_out=p(X))
    refused(b"not in-place", L_out=p(L))
    refused(b"X_out overlaps X", X_out=p(X) + 8 * (n * S - 1))                # the last id the kernel may read
    refused(b"L_out overlaps L", L_out=p(L) + 8)
    refused(b"overlap", L_out=p(Xo) + 8)                                      # the two outputs in one buffer


# ----------------------------------------------------------------------------------------------------------- grid ----
def test_augment_does_not_split_lockstep_units():
    from slnlp import grid
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(48, seq_len=8, src_vocab=40, n_labels=4, seed=3, min_len=3)
    assert "iterator_train__augment" in grid.SHAPE_KEYS_EXCLUDED
    settings = [None, {"frame_drop": 0.1}, {"frame_drop": 0.2, "token_mask": 0.1}]
    cands, folds, tasks, order = grid.build_tasks({"lr": [0.1], "iterator_train__augment": settings}, ds.y, 2)
    units = grid.build_units(cands, folds, tasks, order, lockstep=8)
    assert len(tasks) == 6 and len(units) == 1 and sorted(units[0]) == list(range(6))
