"""GPU: epoch scoring on the device.  ``slnlp_score_rows`` (csrc/score.hip) against its numpy restatement (tests/score_ref.py,
itself held to sklearn on the CPU) with exact equality on all five outputs, and fits whose history carries the old and the new
metric names: every value equal to the score computed on the host from the same epoch's downloaded log-probs."""
import warnings

import numpy as np
import pytest
import torch

from score_ref import counts_ref, make_case, score_ref

pytestmark = pytest.mark.gpu

# (N, V, ld): the smallest call; a row shorter than a wave, N no multiple of four; one column past a wave, padded rows; the
# reference's vocabulary; many strides per lane; more rows than one pass of the grid covers (2048 blocks x 4 rows)
SHAPES = [(1, 1, 1), (5, 37, 37), (257, 65, 80), (64, 202, 202), (9, 5000, 5000), (8197, 3, 4)]


@pytest.mark.parametrize("N,V,ld", SHAPES)
def test_kernel_is_score_ref_exactly(N, V, ld):
    from slnlp import ops
    logp, y, bad = make_case(N, V, seed=N + V)
    ref = score_ref(logp, y)
    buf = torch.full((N, ld), float("nan"), device="cuda")         # padding columns hold NaN: reading one would show
    buf[:, :V] = torch.from_numpy(logp).cuda()
    view, yd = buf[:, :V], torch.from_numpy(y).cuda()
    out = ops.score_buffers(N, V, "cuda")
    for t in out:
        t.view(torch.uint8).fill_(0x5A)                            # whatever was there before: counts must be zeroed by the call
    got = ops.score_rows(view, yd, out=out)
    assert all(a is b for a, b in zip(got, out))
    first = [t.cpu().numpy().copy() for t in out]
    pred, picked, rank, counts = first
    assert np.array_equal(pred, ref[0]), "pred"
    assert np.array_equal(picked.view(np.uint32), ref[1].view(np.uint32)), "picked, bit for bit"
    assert np.array_equal(rank, ref[2]), "rank"
    assert np.array_equal(counts, counts_ref(ref)), "counts"
    assert counts[-1] == len(bad) and (N < 9 or len(bad) == 2)
    # a second call into the same buffers: the same bytes (counts re-zeroed, integer atomics)
    ops.score_rows(view, yd, out=out)
    for a, t in zip(first, out):
        assert a.tobytes() == t.cpu().numpy().tobytes()
    # ... and fresh buffers give them too
    for a, t in zip(first, ops.score_rows(view, yd)):
        assert a.tobytes() == t.cpu().numpy().tobytes()


def test_wrapper_refuses_what_the_kernel_cannot_read():
    from slnlp import ops
    lp, y = torch.zeros(4, 6, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="score_rows"):
        ops.score_rows(lp.double(), y)
    with pytest.raises(ValueError, match="score_rows"):
        ops.score_rows(lp.t(), y[:4])
    with pytest.raises(ValueError, match="score_rows"):
        ops.score_rows(lp, y.int())
    with pytest.raises(ValueError, match="score_rows"):
        ops.score_rows(lp, y, out=ops.score_buffers(5, 6, "cuda"))


# ------------------------------------------------------------------------------------------------------ estimator ----
CFG = dict(module__embedding_size=32, module__num_heads=4, module__num_layers=2, module__hidden_size=64)
RNN_CFG = dict(module__embedding_size=24, module__hidden_size=32, module__num_layers=2)
MODULES = {"tf": ("model.Transformer", CFG), "gru": ("model.EncoderDecoderGRUAttn", RNN_CFG)}
OLD = ["accuracy", "precision_weighted", "recall_weighted", "f1_weighted", "neg_log_loss"]
NEW = ["precision_macro", "recall_macro", "f1_macro", "balanced_accuracy", "top_k_accuracy", "top3_accuracy", "top5_accuracy"]


def dataset():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(80, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)      # 8 output columns, two never a label


def make_net(ds, module, scoring, seed=11, **kw):
    from slnlp.net import NeuralNetClassifier
    mod, cfg = MODULES[module]
    args = dict(module=mod, module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y, module__batch_first=True,
                **cfg, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1, optimizer="torch.optim.SGD",
                optimizer__momentum=0.9, lr=0.05, max_epochs=2, batch_size=20, device="cuda",
                gradient_clipping={"gradient_clip_value": 0.5}, scoring=list(scoring))
    args.update(kw)
    net = NeuralNetClassifier(**args)
    torch.manual_seed(seed)
    return net.initialize()


@pytest.fixture
def epochs_seen(monkeypatch):
    """Every ``end_epoch`` of the test leaves {net id: [per epoch {split: (log-probs on the device, a copy; host labels)}]}."""
    from slnlp import net as net_mod
    seen = {}
    inner = net_mod._FitRun.end_epoch

    def end_epoch(self, tr, va):
        rec = {"train": (tr[1].clone(), np.array(self.train_labels()[1], dtype=np.int64))}
        if va is not None:
            rec["valid"] = (va[1].clone(), np.array(self.va.y, dtype=np.int64))
        seen.setdefault(id(self.net), []).append(rec)
        return inner(self, tr, va)
    monkeypatch.setattr(net_mod._FitRun, "end_epoch", end_epoch)
    return seen


def _old_scores(logp_dev, y):
    """The five reference metrics as before the kernel: ``reduce_epoch``'s torch expression, then the host arithmetic."""
    from slnlp import metrics
    pred, picked = metrics.reduce_epoch(logp_dev, torch.from_numpy(y).to(logp_dev.device))
    return metrics.scores_from_reduction(OLD, y, pred, picked, int(logp_dev.shape[1]))


def _sklearn_scores(logp, y):
    from sklearn.metrics import balanced_accuracy_score, f1_score, precision_score, recall_score, top_k_accuracy_score
    pred, labels = np.argmax(logp, 1), np.arange(logp.shape[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # "y_pred contains classes not in y_true"
        return {"precision_macro": precision_score(y, pred, average="macro", zero_division=0),
                "recall_macro": recall_score(y, pred, average="macro", zero_division=0),
                "f1_macro": f1_score(y, pred, average="macro", zero_division=0),
                "balanced_accuracy": balanced_accuracy_score(y, pred),
                "top_k_accuracy": top_k_accuracy_score(y, logp, k=2, labels=labels),
                "top3_accuracy": top_k_accuracy_score(y, logp, k=3, labels=labels),
                "top5_accuracy": top_k_accuracy_score(y, logp, k=5, labels=labels)}


def _strip(history):
    return [{k: v for k, v in r.items() if k != "dur"} for r in history]


@pytest.mark.parametrize("module", list(MODULES))
def test_history_values_are_the_host_scores_of_the_same_log_probs(module, epochs_seen):
    """A two-epoch fit scoring all old and new names: each history value == the host's number from that epoch's log-probs (new
    names: sklearn on the log-probs; old names: the expression the fit used before).  The same fit inside a lockstep group of
    two: the same history rows."""
    from slnlp.lockstep import fit_lockstep
    ds = dataset()
    solo = make_net(ds, module, OLD + NEW).partial_fit(ds)
    assert len(solo.history) == 2
    for row, rec in zip(solo.history, epochs_seen[id(solo)]):
        assert set(rec) == {"train", "valid"}
        for split, (logp_dev, y) in rec.items():
            want = dict(_old_scores(logp_dev, y), **_sklearn_scores(logp_dev.cpu().numpy(), y))
            for name in OLD + NEW:
                print(f"[{module}] epoch {row['epoch']} {split}_{name}: {row[f'{split}_{name}']!r} (host {want[name]!r})")
                assert row[f"{split}_{name}"] == want[name], (split, name)
    pair = [make_net(ds, module, OLD + NEW), make_net(ds, module, OLD + NEW, seed=12, lr=0.02)]
    fit_lockstep(pair, [ds, ds])
    assert _strip(pair[0].history) == _strip(solo.history)
    assert _strip(pair[1].history) != _strip(solo.history)
    for row, rec in zip(pair[1].history, epochs_seen[id(pair[1])]):                # the other member is scored from its own log-probs
        logp_dev, y = rec["valid"]
        assert row["valid_f1_macro"] == _sklearn_scores(logp_dev.cpu().numpy(), y)["f1_macro"]
        assert row["valid_neg_log_loss"] == _old_scores(logp_dev, y)["neg_log_loss"]


def test_the_five_old_names_alone_keep_their_values(epochs_seen):
    """Only the reference's five names: the history is the one ``reduce_epoch``'s torch expression gives on the same log-probs."""
    ds = dataset()
    net = make_net(ds, "tf", OLD).partial_fit(ds)
    for row, rec in zip(net.history, epochs_seen[id(net)]):
        for split, (logp_dev, y) in rec.items():
            assert {name: row[f"{split}_{name}"] for name in OLD} == _old_scores(logp_dev, y), split
    assert not any(k.endswith("_macro") or "top" in k for k in net.history[0])


def test_a_label_outside_the_columns_raises_naming_split_and_count():
    from slnlp import metrics
    logp, y, bad = make_case(40, 12, seed=1)
    with pytest.raises(ValueError, match=r"train data: 2 of 40 labels"):
        metrics.epoch_scores(["accuracy", "top3_accuracy"], torch.from_numpy(logp).cuda(), torch.from_numpy(y).cuda(), split="train")
