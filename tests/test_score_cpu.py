"""CPU: epoch scoring from the device-side reduction -- the numpy restatement of ``slnlp_score_rows`` against sklearn, the new
scorer names through ``ScoringWrapper``, ``slnlp.metrics`` on CPU tensors, and the C entry's argument checks (no GPU needed:
they run before any HIP call)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from score_ref import counts_ref, make_case, score_ref

NEW = ("precision_macro", "recall_macro", "f1_macro", "balanced_accuracy", "top_k_accuracy", "top1_accuracy", "top5_accuracy",
       "top10_accuracy")
V, N = 14, 240


@pytest.fixture(scope="module")
def case():
    """Finite log-probs on a coarse grid (ties everywhere, forced ones at the maximum and at the true class on both sides of it),
    classes 11-13 absent from y, classes 0 and 13 never predicted."""
    rs = np.random.RandomState(9)
    logp = (np.round(rs.randn(N, V) * 6) / 4 - 4).astype(np.float32)
    y = rs.randint(0, 11, size=N).astype(np.int64)
    logp[:, [0, 13]] = -30.0
    logp[2, 1:13] = -1.0                                    # all equal among the classes that can win
    logp[0, :] = -3.0
    logp[0, [4, 7, 12]] = -0.5                              # ties at the maximum
    y[0] = 7
    y[1] = 6
    logp[1, 1:13] = np.linspace(-9, -1, 12, dtype=np.float32)
    logp[1, [2, 11]] = logp[1, 6]                           # ties at the true class on both sides
    assert np.isfinite(logp).all() and set(np.argmax(logp, 1)) <= set(range(1, 13)) and set(y) == set(range(11))
    return logp, y, score_ref(logp, y)


def _sklearn_scores(logp, y):
    from sklearn.metrics import balanced_accuracy_score, f1_score, precision_score, recall_score, top_k_accuracy_score
    pred = np.argmax(logp, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # "y_pred contains classes not in y_true"
        want = {"precision_macro": precision_score(y, pred, average="macro", zero_division=0),
                "recall_macro": recall_score(y, pred, average="macro", zero_division=0),
                "f1_macro": f1_score(y, pred, average="macro", zero_division=0),
                "balanced_accuracy": balanced_accuracy_score(y, pred),
                "top_k_accuracy": top_k_accuracy_score(y, logp, k=2, labels=np.arange(logp.shape[1]))}
        for k in (1, 5, 10):
            want[f"top{k}_accuracy"] = top_k_accuracy_score(y, logp, k=k, labels=np.arange(logp.shape[1]))
    return want


def test_score_ref_gives_sklearns_numbers_exactly(case):
    """(a) the metrics' arithmetic on ``score_ref``'s outputs == the sklearn functions on the log-probs themselves."""
    from slnlp import metrics
    logp, y, ref = case
    pred, picked, rank = ref[:3]
    assert np.array_equal(pred, np.argmax(logp, 1)) and ref[6] == 0
    assert (ref[3][11:] == 0).all() and ref[4][0] == 0 and ref[4][13] == 0        # absent / never predicted classes are in play
    got = metrics.scores_from_rows(list(NEW), y, pred, picked, rank, counts_ref(ref).astype(np.int64), V)
    want = _sklearn_scores(logp, y)
    for name in NEW:
        print(f"{name}: {got[name]!r} (sklearn {want[name]!r})")
        assert got[name] == want[name], name


class _Fixed:
    def __init__(self, proba):
        from sklearn.base import BaseEstimator, ClassifierMixin

        class Est(ClassifierMixin, BaseEstimator):
            classes_ = np.arange(proba.shape[1])

            def fit(self, X, y):
                return self

            def predict_proba(self, X):
                return proba

            def predict(self, X):
                return proba.argmax(1)
        self.est = Est()


def test_scoring_wrapper_knows_the_new_names():
    """(b) balanced accuracy without ``zero_division``, the top-k family with ``labels=`` and the name's k."""
    from sklearn.metrics import balanced_accuracy_score, precision_score, top_k_accuracy_score
    from slnlp.net import ScoringWrapper
    rs = np.random.RandomState(0)
    proba = rs.dirichlet(np.ones(8), size=40)
    y = rs.randint(0, 7, size=40)                           # class 7 never occurs: labels= must carry it
    labels = list(range(8))
    est = _Fixed(proba).est
    bal = ScoringWrapper("balanced_accuracy", labels)
    top2 = ScoringWrapper("top_k_accuracy", labels)
    top5 = ScoringWrapper("top5_accuracy", labels)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert bal(est, None, y) == balanced_accuracy_score(y, proba.argmax(1))
    assert top2(est, None, y) == top_k_accuracy_score(y, proba, k=2, labels=labels)
    assert top5(est, None, y) == top_k_accuracy_score(y, proba, k=5, labels=labels)
    assert top5(est, None, y) > top2(est, None, y)
    assert bal.greater_is_better and top2.greater_is_better and top5.greater_is_better
    assert (top5.score, repr(top5)) == ("top5_accuracy", "ScoringWrapper('top5_accuracy')")
    assert ScoringWrapper.needs_labels("top5_accuracy") and ScoringWrapper.needs_labels("top_k_accuracy")
    assert ScoringWrapper.needs_labels("neg_log_loss") and not ScoringWrapper.needs_labels("balanced_accuracy")
    # what it did before for the other names stays
    mac = ScoringWrapper("precision_macro", labels)
    assert mac(est, None, y) == precision_score(y, proba.argmax(1), average="macro", zero_division=0)
    assert ScoringWrapper("neg_log_loss", labels).scorer._kwargs == {"labels": labels} and ScoringWrapper("accuracy").scorer._kwargs == {}
    with pytest.raises(ValueError):
        ScoringWrapper("top0_accuracy", labels)            # no such sklearn scorer, and not a k


def test_epoch_scoring_callbacks_translate_the_new_names():
    from slnlp.net import NeuralNetClassifier, ScoringWrapper
    mk = lambda cls_name, **kw: type(cls_name, (), kw)()
    cbs = [mk("EpochScoring", scoring="top5_accuracy", name="valid_top5_accuracy", on_train=False),
           mk("EpochScoring", scoring=ScoringWrapper("balanced_accuracy"), name="train_balanced_accuracy", on_train=True)]
    assert NeuralNetClassifier(module="model.Transformer", callbacks=cbs).get_params()["scoring"] == ["top5_accuracy", "balanced_accuracy"]


def test_metrics_on_cpu_tensors_return_the_new_names(case):
    """(c) ``epoch_scores`` on CPU tensors: the new names, equal to sklearn's numbers; the reduction it rests on equal to ``score_ref``."""
    from slnlp import metrics
    logp, y, ref = case
    got = metrics.epoch_scores(list(NEW), torch.from_numpy(logp), torch.from_numpy(y))
    want = _sklearn_scores(logp, y)
    assert set(got) == set(NEW)
    for name in NEW:
        assert got[name] == want[name], name
    assert all(metrics.is_reduced(n) for n in NEW + metrics.FAST + metrics.REDUCED) and not metrics.is_reduced("roc_auc_ovr")
    assert metrics.top_k_of("top_k_accuracy") == 2 and metrics.top_k_of("top12_accuracy") == 12 and metrics.top_k_of("top0_accuracy") is None
    with pytest.raises(ValueError, match="k=14"):
        metrics.epoch_scores(["top14_accuracy"], torch.from_numpy(logp), torch.from_numpy(y))


@pytest.mark.parametrize("shape", [(1, 1), (5, 37), (40, 65), (13, 300)])
def test_cpu_reduction_is_score_ref(shape):
    """The numpy / torch expression CPU tensors take, against the row-by-row restatement: NaN rows, -inf, labels out of range."""
    from slnlp import metrics
    logp, y, bad = make_case(*shape, seed=shape[0])
    ref = score_ref(logp, y)
    pred, picked, rank, counts = metrics.reduce_rows(torch.from_numpy(logp), torch.from_numpy(y))
    assert pred.dtype == np.int32 and picked.dtype == np.float32 and rank.dtype == np.int32
    assert np.array_equal(pred, ref[0]) and np.array_equal(rank, ref[2])
    assert np.array_equal(picked.view(np.uint32), ref[1].view(np.uint32))
    assert np.array_equal(counts, counts_ref(ref)) and counts[-1] == len(bad)
    assert all(rank[i] == shape[1] and np.isnan(picked[i]) for i in bad)


def test_labels_outside_the_columns_raise_with_split_and_count():
    from slnlp import metrics
    logp, y, bad = make_case(40, 12, seed=1)
    assert len(bad) == 2
    with pytest.raises(ValueError, match=r"valid data: 2 of 40 labels"):
        metrics.epoch_scores(["accuracy"], torch.from_numpy(logp), torch.from_numpy(y), split="valid")


def test_the_five_fast_values_do_not_move(case):
    """(e) the five reference metrics: the same floats whether or not new names ride along, and the same as the expression
    ``reduce_epoch`` + ``scores_from_reduction`` has always given."""
    from slnlp import metrics
    logp, y, _ = case
    lp, yt = torch.from_numpy(logp), torch.from_numpy(y)
    alone = metrics.epoch_scores(list(metrics.FAST), lp, yt)
    mixed = metrics.epoch_scores(list(NEW[:3]) + list(metrics.FAST) + list(NEW[3:]), lp, yt, y_host=y)
    pred, picked = metrics.reduce_epoch(lp, yt)
    old = metrics.scores_from_reduction(list(metrics.FAST), y, pred, picked, V)
    assert list(alone) == list(metrics.FAST)
    for name in metrics.FAST:
        assert alone[name] == mixed[name] == old[name], name
    # the 0.0 / -1e3 row of the log-loss clip case included
    logp2, y2, _ = make_case(8, 6, seed=2)
    lp2, yt2 = torch.from_numpy(logp2), torch.from_numpy(y2)
    pred, picked = metrics.reduce_epoch(lp2, yt2)
    assert metrics.epoch_scores(list(metrics.FAST), lp2, yt2) == metrics.scores_from_reduction(list(metrics.FAST), y2, pred, picked, 6)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    return _lib.load()


def test_score_rows_argument_errors_are_codes_with_a_message(lib):
    """(d) every refusal returns SLNLP_ERR_INVALID_ARG with a text naming score_rows, before any HIP call."""
    n, v, ld = 6, 5, 8
    logp = np.zeros((n, ld), np.float32)
    y = np.zeros(n, np.int64)
    pred, picked, rank = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    counts = np.zeros(3 * v + 1, np.int32)
    p = lambda a: a.ctypes.data
    good = dict(logp=p(logp), ld=ld, y=p(y), N=n, V=v, pred=p(pred), picked=p(picked), rank=p(rank), counts=p(counts))

    def refused(word, **change):
        a = dict(good, **change)
        rc = lib.slnlp_score_rows(a["logp"], a["ld"], a["y"], a["N"], a["V"], a["pred"], a["picked"], a["rank"], a["counts"], None)
        msg = lib.slnlp_last_error()
        assert rc == 1, (change, rc)
        assert b"score_rows" in msg and word in msg, (change, msg)

    for name in ("logp", "y", "pred", "picked", "rank", "counts"):
        refused(b"null", **{name: None})
    refused(b"N=0", N=0)
    refused(b"N=-3", N=-3)
    refused(b"V=0", V=0)
    refused(b"V=-1", V=-1)
    refused(b"ld=4", ld=4)                                  # ld < V
    refused(b"N=2147483648", N=1 << 31)                     # beyond an int32 row index
    refused(b"V=715827883", V=(2 ** 31 - 2) // 3 + 1, ld=1 << 30)        # 3 V + 1 counts beyond int32
    refused(b"overlaps input logp", pred=p(logp) + 4 * (ld * (n - 1) + v - 1))     # the last float the kernel reads
    refused(b"overlaps input y", counts=p(y) + 8)
    refused(b"overlaps input logp", picked=p(logp))
    refused(b"overlap", rank=p(pred))                       # two outputs in one buffer
