"""CPU: the shuffled train order (slnlp/sampler.py) against torch's own sampler classes, its place in the history, the
config / grid names of the two ``iterator_train__*`` keys, and train metrics paired in visit order."""
import glob
import os
import warnings

import numpy as np
import pytest
import torch
from torch.utils.data import BatchSampler, RandomSampler

from slnlp import cli, grid, metrics, sampler
from slnlp.data import synthetic_dataset

HERE = os.path.dirname(os.path.abspath(__file__))
# (n, batch_size, drop_last, seed): n % batch_size == 0, a short last batch, n < batch_size without drop_last, n == 1, a 63-bit seed
CASES = [(200, 50, False, 1), (200, 50, True, 1), (64, 20, False, 7), (64, 20, True, 7), (13, 50, False, 3), (1, 4, False, 0),
         (1, 1, True, 5), (101, 10, True, 2 ** 62 + 12345), (37, 37, False, 11)]


def torch_epochs(n, batch_size, drop_last, seed, epochs):
    """The oracle: ``epochs`` iterations of torch's own classes, each flattened."""
    gen = torch.Generator().manual_seed(seed)
    batches = BatchSampler(RandomSampler(range(n), generator=gen), batch_size, drop_last)
    return [np.array([i for b in batches for i in b], dtype=np.int64) for _ in range(epochs)]


@pytest.mark.parametrize("n,batch_size,drop_last,seed", CASES)
def test_epoch_order_is_torchs_batch_sampler_over_random_sampler(n, batch_size, drop_last, seed):
    want = torch_epochs(n, batch_size, drop_last, seed, 3)
    eo = sampler.EpochOrder(n, batch_size, seed, drop_last)
    n_visit = (n // batch_size) * batch_size if drop_last else n
    assert eo.n_visit == n_visit == sampler.n_visit(n, batch_size, drop_last)
    for e in range(3):
        got = eo.next_epoch()
        assert got.dtype == np.int64 and got.shape == (n_visit,)
        assert np.array_equal(got, want[e]), (e, got, want[e])
        assert len(set(got.tolist())) == n_visit and (n_visit == 0 or (0 <= got.min() and got.max() < n))


def test_the_order_is_a_real_permutation_that_changes_per_epoch():
    eo = sampler.EpochOrder(200, 50, 1)
    a, b = eo.next_epoch(), eo.next_epoch()
    assert not np.array_equal(a, np.arange(200)) and not np.array_equal(a, b)
    assert sorted(a.tolist()) == sorted(b.tolist()) == list(range(200))
    assert not np.array_equal(a, sampler.EpochOrder(200, 50, 2).next_epoch())          # the seed matters


def test_drop_last_without_a_full_batch_is_an_error():
    with pytest.raises(ValueError, match="drop_last"):
        sampler.EpochOrder(13, 50, 1, drop_last=True)


@pytest.mark.parametrize("k", [0, 1, 4])
def test_fast_forward_lands_on_epoch_k(k):
    want = torch_epochs(64, 20, False, 9, k + 1)[k]
    assert np.array_equal(sampler.EpochOrder(64, 20, 9).fast_forward(k).next_epoch(), want)


def test_a_history_restores_seed_and_position():
    hist = [{"epoch": 1, "shuffle_seed": 77}, {"epoch": 2, "shuffle_seed": 77}]
    assert sampler.seed_from_history(hist) == 77
    assert sampler.seed_from_history([{"epoch": 1}]) is None and sampler.seed_from_history([]) is None
    eo = sampler.EpochOrder(64, 20, sampler.seed_from_history(hist)).fast_forward(len(hist))
    assert np.array_equal(eo.next_epoch(), torch_epochs(64, 20, False, 77, 3)[2])


def test_seed_draw_is_random_samplers_and_repeats_under_a_seed():
    torch.manual_seed(5)
    a = sampler.draw_seed()
    torch.manual_seed(5)
    want = int(torch.empty((), dtype=torch.int64).random_().item())                     # torch/utils/data/sampler.py, generator None
    assert a == want and isinstance(a, int)
    assert sampler.draw_seed() != a


def test_check_order_rejects_what_the_device_would_not_survive():
    assert sampler.check_order([2, 0, 1], 3, 3).dtype == np.int64
    for bad, rows, n in [([0, 3], 3, 2), ([-1, 0], 3, 2), ([0, 1], 3, 3), ([[0, 1]], 3, None), ([], 3, None)]:
        with pytest.raises(ValueError):
            sampler.check_order(bad, rows, n)


# ------------------------------------------------------------------------------------------------- config surface ----
def test_cli_prefixes_iterator_train_args():
    ds = synthetic_dataset(30, seq_len=6, src_vocab=20, n_labels=3, seed=2, min_len=2)
    base = {"model": "model.Transformer", "optimizer_args": {"momentum": 0.9}}
    p = cli.build_net_params(dict(base, iterator_train_args={"shuffle": True, "drop_last": False}), ds, "cuda")
    assert p["iterator_train__shuffle"] is True and p["iterator_train__drop_last"] is False
    assert not [k for k in cli.build_net_params(base, ds, "cuda") if k.startswith("iterator_")]
    g = cli.build_param_grid({"lr": [0.1], "iterator_train_args": {"shuffle": [False, True]}, "optimizer_args": {"nesterov": [True]}})
    assert g == {"optimizer__nesterov": [True], "iterator_train__shuffle": [False, True], "lr": [0.1]}
    assert cli.build_param_grid({"iterator_train_args": {"drop_last": True}}) == {"iterator_train__drop_last": [True]}
    assert "iterator_train_args" in cli.DICT_ARGS


def test_reference_configs_are_untouched_by_the_new_key():
    from sklearn.model_selection import ParameterGrid
    files = sorted(glob.glob(os.path.join(HERE, "golden", "reference_configs", "config-*.yaml")))
    assert len(files) == 3
    ds = synthetic_dataset(30, seq_len=6, src_vocab=20, n_labels=3, seed=2, min_len=2)
    for f in files:
        args = cli.load_config(f)
        g = cli.build_param_grid(args["grid_args"])
        # 3 lr x 3 embedding sizes x 3 hidden sizes x 3 depths x 2 dropout rates, x 2 head counts for the Transformer only
        assert len(ParameterGrid(g)) == (324 if f.endswith("config-transformer.yaml") else 162), f
        assert not [k for k in list(g) + list(cli.build_net_params(args, ds, "cuda")) if k.startswith("iterator_")], f


def test_estimator_checks_the_two_keys_it_honours():
    from slnlp.net import NeuralNetClassifier
    net = NeuralNetClassifier("model.Transformer", iterator_train__shuffle=True, iterator_train__collate_fn=None)
    assert net._iterator_train() == (True, False)
    assert NeuralNetClassifier("model.Transformer")._iterator_train() == (False, False)
    assert NeuralNetClassifier("model.Transformer", iterator_train__drop_last=np.bool_(True))._iterator_train() == (False, True)
    for key in ("shuffle", "drop_last"):
        with pytest.raises(ValueError, match=key):
            NeuralNetClassifier("model.Transformer", **{f"iterator_train__{key}": "yes"})._iterator_train()


# ----------------------------------------------------------------------------------------------------------- grid ----
def test_shuffle_does_not_split_lockstep_units_and_drop_last_does():
    ds = synthetic_dataset(48, seq_len=8, src_vocab=40, n_labels=4, seed=3, min_len=3)
    assert "iterator_train__shuffle" in grid.SHAPE_KEYS_EXCLUDED and "iterator_train__drop_last" not in grid.SHAPE_KEYS_EXCLUDED
    cands, folds, tasks, order = grid.build_tasks({"lr": [0.1, 0.01], "iterator_train__shuffle": [False, True]}, ds.y, 2)
    units = grid.build_units(cands, folds, tasks, order, lockstep=8)
    assert len(tasks) == 8 and len(units) == 1 and sorted(units[0]) == list(range(8))
    cands, folds, tasks, order = grid.build_tasks({"lr": [0.1, 0.01], "iterator_train__drop_last": [False, True]}, ds.y, 2)
    units = grid.build_units(cands, folds, tasks, order, lockstep=8)
    assert len(units) == 2
    for u in units:
        assert len({cands[tasks[t][0]]["iterator_train__drop_last"] for t in u}) == 1 and len(u) == 4


# -------------------------------------------------------------------------------------------------------- metrics ----
def test_train_metrics_in_visit_order_equal_the_sklearn_scorers_on_the_permuted_inputs():
    """A shuffled epoch's log-probs lie in visit order and are scored against the labels in visit order: the fast metrics on the
    permuted (y, pred, picked) are the sklearn scorers' numbers on the same permuted inputs."""
    from slnlp.net import ScoringWrapper, _CachedPredictor
    for seed, (N, V) in enumerate([(600, 202), (37, 16)]):
        rng = np.random.RandomState(seed)
        y = rng.randint(2, V, N)
        logits = (rng.randn(N, V) * 3).astype(np.float32)
        logits[np.arange(N)[::3], y[::3]] += 6.0
        logp = torch.log_softmax(torch.from_numpy(logits), -1)
        order = sampler.EpochOrder(N, 50, seed + 1).next_epoch()
        y_v, logp_v = y[order], logp[torch.from_numpy(order)]
        pred, picked = metrics.reduce_epoch(logp_v, torch.from_numpy(y_v))
        assert np.array_equal(pred, logp.argmax(1).numpy()[order])
        fast = metrics.scores_from_reduction(list(metrics.FAST), y_v.astype(np.int64), pred, picked, V)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for name in metrics.FAST:
                ref = float(ScoringWrapper(name, list(range(V)))(_CachedPredictor(np.exp(logp_v.numpy()), np.arange(V)), None, y_v))
                assert fast[name] == ref, (name, fast[name], ref)
