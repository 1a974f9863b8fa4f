"""CPU: the host side of the reliability diagnostics -- the numpy restatement the GPU tests lean on (tests/reliability_ref.py)
against a direct fp64 softmax and a plain loop over the bin masks, its edge rules, the metric names, ``ScoringWrapper``,
``metrics.epoch_scores`` on CPU tensors, the grid / CLI pass-through and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest
import torch

from reliability_ref import bin_of, reliability_ref, rows_ref, summary_ref, table_ref
from test_calibration_cpu import make_logp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(257, 70, 8.0, 0.6), (257, 70, 0.3, 0.9), (5, 3, 2.0, 0.6), (33, 129, 4.0, 0.6), (300, 202, 3.0, 0.5)]
INPUTS = [(c, seed) for c in CASES for seed in (1, 2, 3)]


def _softmax64(logp, beta=1.0):
    z = beta * logp.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------------------------------------------- restatement ----
@pytest.mark.parametrize("beta", [1.0, 0.16, 6.25])
@pytest.mark.parametrize("case,seed", INPUTS)
def test_rows_against_a_direct_computation(case, seed, beta):
    logp, y = make_logp(*case, seed)
    rows = rows_ref(logp, y, 15, beta)
    p = _softmax64(logp, beta)
    idx = np.arange(len(y))
    brier = ((p - np.eye(p.shape[1])[y]) ** 2).sum(axis=1)
    with np.errstate(divide="ignore"):
        nll = -np.log(p[idx, y])
    seen = np.isfinite(nll)                                 # (beta 6.25 at scale 8: p_y underflows in the direct form only)
    d_conf, d_brier = np.abs(rows[:, 0] - p.max(axis=1)).max(), np.abs(rows[:, 1] - brier).max()
    d_nll = (np.abs(rows[seen, 2] - nll[seen]) / np.maximum(1.0, nll[seen])).max()
    print(f"[{case} seed {seed} beta {beta}] conf {d_conf:.2e} brier {d_brier:.2e} nll {d_nll:.2e}")
    assert max(d_conf, d_brier, d_nll) <= 1e-12
    assert np.array_equal(rows[:, 3], 2.0 * bin_of(rows[:, 0], 15) + (logp.argmax(axis=1) == y))


@pytest.mark.parametrize("bins", [1, 10, 15, 64])
@pytest.mark.parametrize("case,seed", INPUTS)
def test_ece_against_a_plain_loop_over_the_bin_masks(case, seed, bins):
    logp, y = make_logp(*case, seed)
    got = reliability_ref(logp, y, bins)
    p = _softmax64(logp)
    conf, correct = p.max(axis=1), (logp.argmax(axis=1) == y).astype(np.float64)
    ece, mce = 0.0, 0.0
    for b in range(bins):
        lo, hi = b / bins, (b + 1) / bins
        m = (conf > lo) & (conf <= hi)
        if m.any():
            gap = abs(correct[m].mean() - conf[m].mean())
            ece += gap * m.sum() / len(y)
            mce = max(mce, gap)
    idx = np.arange(len(y))
    assert abs(got["ece"] - ece) <= 1e-12 and abs(got["mce"] - mce) <= 1e-12
    assert abs(got["brier"] - ((p - np.eye(p.shape[1])[y]) ** 2).sum(axis=1).mean()) <= 1e-12
    assert abs(got["nll"] + np.log(p[idx, y]).mean()) <= 1e-12 * max(1.0, got["nll"])
    assert abs(got["accuracy"] - correct.mean()) <= 1e-15 and abs(got["confidence"] - conf.mean()) <= 1e-12
    assert (got["rows"], got["bad_labels"], got["nan_rows"]) == (len(y), 0, 0)


def test_the_two_big_cases_sit_where_the_issue_says():
    """An overconfident model's confidence lies above its accuracy, an underconfident one's below; temperature helps the first."""
    from calibration_ref import fit_temperature_ref
    over, under = make_logp(257, 70, 8.0, 0.6, 1), make_logp(257, 70, 0.3, 0.9, 1)
    a, b = reliability_ref(*over), reliability_ref(*under)
    assert a["confidence"] > a["accuracy"] + 0.1 and b["confidence"] < b["accuracy"] - 0.1
    beta = fit_temperature_ref(*over)["beta"]
    assert reliability_ref(*over, beta=beta)["ece"] < a["ece"] and reliability_ref(*over, beta=beta)["nll"] < a["nll"]
    assert (rows_ref(*over, 15)[:, 0] == 1.0).sum() > 0, "saturated rows are part of the overconfident family"


def test_table_order_is_a_sum():
    rows = rows_ref(*make_logp(300, 202, 3.0, 0.5, 2), 10)
    t = table_ref(rows, 10)
    code = rows[:, 3].astype(int)
    assert np.array_equal(t[:10, 0], np.bincount(code >> 1, minlength=10)) and t[:10, 0].sum() == 300
    assert np.array_equal(t[:10, 2], np.bincount(code >> 1, weights=code & 1, minlength=10))
    assert np.allclose(t[:10, 1], np.bincount(code >> 1, weights=rows[:, 0], minlength=10), rtol=1e-14, atol=0)
    assert abs(t[10, 0] - rows[:, 1].sum()) <= 1e-12 * rows[:, 1].sum() and np.array_equal(t[10, 2:], [0.0, 0.0])
    assert np.array_equal(t[:, 3][:10], np.zeros(10))


# ----------------------------------------------------------------------------------------------------- edge rules ----
def test_edge_rules():
    # conf == 1.0 exactly (the other columns vanish) and the largest conf below 1 that 1 / (1 + rest) reaches: both in the top
    # bin, whatever B -- as is the double one ulp below 1, whatever produced it (bin_of, below)
    sat = np.array([[0.0, -200.0, -300.0], [0.0, np.log(2.0 ** -52), -300.0]], dtype=np.float32)
    for bins in (1, 2, 10, 15, 64):
        rows = rows_ref(sat, np.array([0, 1]), bins)
        assert rows[0, 0] == 1.0 and 1.0 - 2.0 ** -51 <= rows[1, 0] < 1.0, rows[:, 0]
        assert np.array_equal(rows[:, 3], [2.0 * (bins - 1) + 1.0, 2.0 * (bins - 1)])
    assert bin_of(1.0, 15) == 14 and bin_of(np.nextafter(1.0, 0.0), 15) == 14 and bin_of(14 / 15, 15) == 13
    assert bin_of(0.0, 15) == 0 and bin_of(1e-300, 15) == 0 and bin_of(0.5, 2) == 0 and bin_of(np.nextafter(0.5, 1.0), 2) == 1
    # B = 1: one bin, ECE = |accuracy - confidence|
    logp, y = make_logp(33, 7, 2.0, 0.6, 4)
    one = reliability_ref(logp, y, 1)
    assert abs(one["ece"] - abs(one["accuracy"] - one["confidence"])) <= 1e-15 and abs(one["ece"] - one["mce"]) <= 1e-15
    # V = 2 with equal columns: conf = 0.5, pred = the first column, brier = 0.5, nll = ln 2
    half = np.full((2, 2), np.log(0.5), dtype=np.float32)
    rows = rows_ref(half, np.array([0, 1]), 10)
    assert np.array_equal(rows[:, 0], [0.5, 0.5]) and np.array_equal(rows[:, 3], [2 * 4 + 1.0, 2 * 4.0])
    assert np.array_equal(rows[:, 1], [0.5, 0.5]) and np.allclose(rows[:, 2], np.log(2.0), rtol=1e-15)
    # a bad label: counted, never an index, out of every sum
    bad = y.copy()
    bad[3], bad[20] = -1, 7
    keep = np.ones(33, dtype=bool)
    keep[[3, 20]] = False
    got, want = reliability_ref(logp, bad), reliability_ref(logp[keep], y[keep])
    assert got["bad_labels"] == 2 and got["rows"] == 31 and np.array_equal(rows_ref(logp, bad, 15)[3], [0.0, 0.0, 0.0, -1.0])
    assert all(abs(got[k] - want[k]) <= 1e-15 for k in ("ece", "mce", "brier", "nll", "accuracy", "confidence"))
    # a NaN row, a row whose maximum is not finite: code -2, NaN terms, the four scores NaN, the means over the rest
    for poison in (np.nan, np.inf):
        broken = logp.copy()
        broken[5, 2] = poison
        rows = rows_ref(broken, y, 15)
        assert rows[5, 3] == -2.0 and np.isnan(rows[5, :3]).all() and not np.isnan(np.delete(rows, 5, axis=0)).any()
        got = reliability_ref(broken, y)
        assert got["nan_rows"] == 1 and got["rows"] == 32 and all(np.isnan(got[k]) for k in ("ece", "mce", "brier", "nll"))
        assert np.isfinite(got["accuracy"]) and np.isfinite(got["confidence"])
    dead = logp.copy()
    dead[6] = -np.inf
    assert rows_ref(dead, y, 15)[6, 3] == -2.0
    # a -inf column in an otherwise fine row is probability 0
    hole = logp.copy()
    hole[7, (y[7] + 1) % 7] = -np.inf
    rows = rows_ref(hole, y, 15)
    assert rows[7, 3] >= 0 and np.isfinite(rows[7]).all()


# ---------------------------------------------------------------------------------------------------- the metrics ----
def test_metric_names():
    from slnlp import metrics
    assert metrics.CALIBRATION == ("neg_ece", "neg_mce", "neg_brier")
    assert metrics.FAST == ("accuracy", "precision_weighted", "recall_weighted", "f1_weighted", "neg_log_loss")
    assert metrics.REDUCED == ("precision_macro", "recall_macro", "f1_macro", "balanced_accuracy", "top_k_accuracy")
    for name in metrics.CALIBRATION + ("neg_ece1", "neg_ece10", "neg_ece64"):
        assert metrics.is_reduced(name), name
    assert metrics.calibration_metric_of("neg_ece") == ("ece", 15) and metrics.calibration_metric_of("neg_ece64") == ("ece", 64)
    assert metrics.calibration_metric_of("neg_mce") == ("mce", 15) and metrics.calibration_metric_of("neg_brier") == ("brier", None)
    for name in ("neg_ece0", "neg_ece65", "neg_ece015", "neg_ece100"):
        with pytest.raises(ValueError, match="bins"):
            metrics.is_reduced(name)
    for name in ("ece", "neg_ece_15", "neg_mce10", "neg_brier_score", "neg_ece-1", None):
        assert metrics.calibration_metric_of(name) is None and not metrics.is_reduced(name)


@pytest.mark.parametrize("case,seed", [(CASES[0], 1), (CASES[1], 2), (CASES[2], 3)])
def test_numpy_implementation_on_probabilities(case, seed):
    """``metrics.reliability_numpy`` renormalises its rows in fp64; on fp64 probabilities it is the restatement."""
    from slnlp import metrics
    logp, y = make_logp(*case, seed)
    for bins in (1, 10, 15, 64):
        got = metrics.reliability_from_table(metrics.reliability_numpy(_softmax64(logp), y, bins)[1])
        want = reliability_ref(logp, y, bins)
        for k in ("ece", "mce", "brier", "nll", "accuracy", "confidence"):
            assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (bins, k, got[k], want[k])
        assert (got["rows"], got["bad_labels"], got["nan_rows"]) == (len(y), 0, 0)
        table = table_ref(rows_ref(logp, y, bins), bins)
        assert np.array_equal(got["bins"]["count"], table[:bins, 0].astype(np.int64)) and got["bins"]["count"].dtype == np.int64
        filled = table[:bins, 0] > 0
        assert np.isnan(got["bins"]["confidence"][~filled]).all() and np.isnan(got["bins"]["accuracy"][~filled]).all()
        assert np.allclose(got["bins"]["confidence"][filled], table[:bins, 1][filled] / table[:bins, 0][filled], rtol=1e-12, atol=0)
    for bins in (0, 65, 2.5, True, None):
        with pytest.raises(ValueError, match="bins"):
            metrics.reliability_numpy(_softmax64(logp), y, bins)


def test_from_table_agrees_with_the_restated_summary():
    from slnlp import metrics
    logp, y = make_logp(257, 70, 8.0, 0.6, 3)
    y[4] = 70
    for poison in (False, True):
        if poison:
            logp[9, 0] = np.nan
        table = table_ref(rows_ref(logp, y, 15), 15)
        got, want = metrics.reliability_from_table(table), summary_ref(table)
        for k, v in want.items():
            assert got[k] == v or (np.isnan(got[k]) and np.isnan(v)) or abs(got[k] - v) <= 1e-15, (k, got[k], v)
        assert got["bad_labels"] == 1 and got["nan_rows"] == int(poison)


class _Fixed:
    """An estimator that predicts what it is told (what ``_CachedPredictor`` is to EpochScoring)."""

    def __init__(self, proba):
        from slnlp.net import _CachedPredictor
        self.est = _CachedPredictor(proba, np.arange(proba.shape[1]))


@pytest.mark.parametrize("name,key,bins", [("neg_ece", "ece", 15), ("neg_ece10", "ece", 10), ("neg_ece64", "ece", 64), ("neg_mce", "mce", 15),
                                           ("neg_brier", "brier", 15)])
def test_scoring_wrapper(name, key, bins):
    from slnlp import metrics
    from slnlp.net import ScoringWrapper
    logp, y = make_logp(257, 70, 8.0, 0.6, 1)
    proba = _softmax64(logp).astype(np.float32)             # what predict_proba hands a scorer
    labels = list(range(70))
    wr = ScoringWrapper(name, labels)
    assert wr.greater_is_better is False and wr.scorer._sign == -1 and wr.score == name
    assert repr(wr) == f"ScoringWrapper('{name}')" and ScoringWrapper.needs_labels(name)
    got = wr(_Fixed(proba).est, None, y)
    # the restatement ON THE SAME PROBABILITIES: their fp64 logarithms renormalise to the same rows up to rounding
    p64 = proba.astype(np.float64)
    p64 /= p64.sum(axis=1, keepdims=True)
    rows = metrics.reliability_numpy(proba, y, bins)[0]
    conf, correct = p64.max(axis=1), proba.argmax(axis=1) == y
    want = {"brier": ((p64 - np.eye(70)[y]) ** 2).sum(axis=1).mean()}
    gaps = [(abs(correct[m].sum() - conf[m].sum()), m.sum()) for m in (bin_of(conf, bins) == b for b in range(bins)) if m.any()]
    want["ece"], want["mce"] = sum(g for g, _ in gaps) / len(y), max(g / n for g, n in gaps)
    print(f"{name}: {got!r} (restated {-want[key]!r})")
    assert abs(got + want[key]) <= 1e-12 and got <= 0.0
    assert np.array_equal(rows[:, 3], 2.0 * bin_of(rows[:, 0], bins) + correct)
    with pytest.raises(ValueError, match="labels lie outside"):
        wr(_Fixed(proba).est, None, np.where(np.arange(257) == 3, 70, y))
    # columns that stand for other class ids than 0 .. V - 1: the label set says which
    shifted = ScoringWrapper(name, [10 + c for c in labels])
    assert shifted(_Fixed(proba).est, None, y + 10) == got


@pytest.mark.parametrize("name,key", [("neg_ece", "ece"), ("neg_ece4", "ece"), ("neg_mce", "mce"), ("neg_brier", "brier")])
def test_scoring_wrapper_with_two_classes(name, key):
    """With two classes sklearn's ``predict_proba`` scorers pass the second column alone: the wrapper scores what it would score on
    both columns, and what the restatement gives on their logarithms."""
    from slnlp import metrics
    from slnlp.net import ScoringWrapper
    logp, y = make_logp(40, 2, 2.0, 0.6, 3)
    proba = _softmax64(logp).astype(np.float32)
    got = ScoringWrapper(name, [0, 1])(_Fixed(proba).est, None, y)
    bins = metrics.calibration_metric_of(name)[1]
    both = proba.astype(np.float64)
    both[:, 0] = 1.0 - both[:, 1]                           # the two columns as the scorer rebuilds them
    assert got == -metrics.calibration_error(y, both, kind=key, bins=bins, labels=[0, 1])
    assert got == -metrics.calibration_error(y, proba[:, 1], kind=key, bins=bins)
    want = reliability_ref(np.log(both).astype(np.float32), y, bins or 15)[key]
    print(f"{name}: {got!r} (restated {-want!r})")
    assert abs(got + want) <= 1e-6 and got < 0.0           # float32 log-probs of float32 probabilities: 1e-7 apiece
    shifted = ScoringWrapper(name, [3, 8])(_Fixed(proba).est, None, np.where(y == 1, 8, 3))
    assert shifted == got


@pytest.mark.parametrize("name", ["neg_ece0", "neg_ece65"])
def test_scoring_wrapper_rejects_bin_counts_out_of_range(name):
    from slnlp.net import ScoringWrapper
    with pytest.raises(ValueError, match="bins"):
        ScoringWrapper(name, [0, 1])


def test_epoch_scores_on_cpu_tensors():
    from slnlp import metrics
    logp, y = make_logp(257, 70, 8.0, 0.6, 2)
    names = ["accuracy", "neg_ece", "neg_ece10", "neg_mce", "neg_brier", "neg_log_loss", "roc_auc_ovr"]
    got = metrics.epoch_scores(names, torch.from_numpy(logp), torch.from_numpy(y), split="valid")
    assert list(got) == ["accuracy", "neg_log_loss", "neg_ece", "neg_ece10", "neg_mce", "neg_brier"]
    r15, r10 = reliability_ref(logp, y, 15), reliability_ref(logp, y, 10)
    for name, want in (("neg_ece", -r15["ece"]), ("neg_ece10", -r10["ece"]), ("neg_mce", -r15["mce"]), ("neg_brier", -r15["brier"])):
        assert abs(got[name] - want) <= 1e-12, (name, got[name], want)
    assert got["accuracy"] == r15["accuracy"]
    assert metrics.epoch_scores(["accuracy"], torch.from_numpy(logp), torch.from_numpy(y)) == {"accuracy": got["accuracy"]}
    y[5] = 70
    for some in (["neg_brier"], ["accuracy", "neg_ece"]):
        with pytest.raises(ValueError, match="scoring the valid data: 1 of 257 labels lie outside the 70 classes"):
            metrics.epoch_scores(some, torch.from_numpy(logp), torch.from_numpy(y), split="valid")


# ---------------------------------------------------------------------------------------------------- grid, CLI ----
def _ece_fit_and_score(factory, params, train, test, scoring):
    """Stands in for a fit: 'predicts' seeded probabilities whose sharpness is the candidate's lr, scored by the grid's scorer."""
    from slnlp.net import ScoringWrapper
    V = len(train.vocab_y)
    logp = make_logp(len(test), V, 10.0 * params["lr"], 0.6, 7)[0]
    wr = ScoringWrapper(scoring, train.labels() if ScoringWrapper.needs_labels(scoring) else None)
    return float(wr(_Fixed(_softmax64(logp).astype(np.float32)).est, test, test.y))


def test_grid_ranks_on_the_new_names():
    from slnlp import grid
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(48, seq_len=8, src_vocab=40, n_labels=4, seed=3, min_len=3)
    gs = grid.ShardedGridSearchCV(lambda: None, {"lr": [0.01, 0.5]}, cv=2, scoring="neg_ece", fit_and_score=_ece_fit_and_score,
                                  refit=False).fit(ds)
    scores = gs.cv_results_["mean_test_score"]
    assert np.isfinite(scores).all() and (scores <= 0.0).all() and scores[0] != scores[1]
    assert gs.best_index_ == int(np.argmax(scores))         # the negated error: greater is better, as for neg_log_loss
    # the names are no shape key of their own: they travel in the estimator's ``scoring`` list and do not regroup anything
    cands, folds, tasks, order = grid.build_tasks({"lr": [0.1, 0.2]}, ds.y, 2)
    assert len(grid.build_units(cands, folds, tasks, order, lockstep=8)) == 1


def test_cli_passes_the_names_through():
    from slnlp import cli

    class _Vocab:
        stoi = {"<pad>": 1}

    class _Data:
        vocab_X = vocab_y = _Vocab()
    base = {"model": "model.Transformer"}
    assert cli.build_net_params(dict(base, scoring="neg_ece"), _Data(), "cuda")["scoring"] == ["neg_ece"]
    both = cli.build_net_params(dict(base, scoring=["neg_ece20", "neg_brier", "accuracy"]), _Data(), "cuda")["scoring"]
    assert both == ["neg_ece20", "neg_brier", "accuracy"]
    assert cli.SCALAR_ARGS["scoring"] is str


def test_estimator_surface_without_a_gpu():
    from slnlp.net import NeuralNetClassifier
    net = NeuralNetClassifier(module="model.Transformer", scoring=["neg_ece", "neg_brier"])
    assert net.get_params()["scoring"] == ["neg_ece", "neg_brier"] and callable(net.reliability)
    with pytest.raises(RuntimeError, match="not initialized"):
        net.reliability(None)
    # calibration's own options are what they were
    with pytest.raises(ValueError, match="calibration"):
        NeuralNetClassifier(module="model.Transformer", calibration={"method": "temperature", "bins": 10}).initialize()


# ----------------------------------------------------------------------------------------------------------- C ABI ----
def test_the_entry_point_is_declared_and_bound():
    from slnlp import _lib, metrics, ops
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                  # the way tests/test_abi.py reads the header
    declared = set(re.findall(r"\b(slnlp_[a-z0-9_]+)\s*\(", src))
    assert "slnlp_reliability_rows" in declared and "slnlp_reliability_rows" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["slnlp_reliability_rows"][1]) == 10
    (bins,), = [re.findall(r"#define SLNLP_REL_MAX_BINS (\d+)", src)]
    assert int(bins) == 64 == _lib.REL_MAX_BINS == metrics.MAX_BINS
    assert callable(ops.reliability_rows) and callable(ops.reliability_download)
    hip = open(os.path.join(ROOT, "sign-language-nlp_amd", "csrc", "reliability.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", hip), "the table is summed in a fixed order, without atomics"
    assert "csrc/reliability.hip" in open(os.path.join(ROOT, "sign-language-nlp_amd", "Makefile")).read()
