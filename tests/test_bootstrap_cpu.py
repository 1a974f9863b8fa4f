"""CPU: the host side of the bootstrap of the scores -- the numpy restatement the GPU tests lean on (tests/bootstrap_ref.py) against
sklearn on explicitly resampled arrays, the quality of the draw, the bootstrap standard deviation against the binomial one, the
summarisers ``metrics.bootstrap_intervals`` / ``bootstrap_difference`` against direct ``np.quantile``, the options of the estimator
and the CLI, and the C ABI's declarations.

The two statistical checks are deterministic: SEED below is a seed for which the restatement passes them (the first one tried; the
bounds are wide -- 5 binomial standard deviations, and six times the estimate's own relative error)."""
import os
import re

import numpy as np
import pytest

from bootstrap_ref import FIXED, STAGE, bootstrap_ref, column_names, draws, make_case, recount, replicate_scores
from test_calibration_cpu import make_logp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261018


# ---------------------------------------------------------------------------------------------------- restatement ----
def test_replicates_against_sklearn_on_resampled_arrays():
    """A case with rare classes: 300 rows over 202 classes, so a resample loses classes and meets some in the predictions only."""
    import warnings

    import torch
    from sklearn.metrics import (accuracy_score, balanced_accuracy_score, precision_recall_fscore_support, top_k_accuracy_score)
    from slnlp import metrics
    logp, y = make_logp(300, 202, 3.0, 0.5, 2)
    V, k, B = 202, 5, 4
    pred, _, rank, _ = metrics.reduce_rows(torch.from_numpy(logp), torch.from_numpy(y))
    values = np.random.RandomState(0).randn(300, 3)
    stats, counts = bootstrap_ref(y, pred, rank, values, V, k, B, SEED)
    rows = draws(300, B, SEED)
    lost = 0
    for b in range(B):
        yb, pb = y[rows[b]], pred[rows[b]].astype(np.int64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                  # (balanced_accuracy_score: y_pred holds classes that y_true lacks)
            want = [accuracy_score(yb, pb)]
            want += [precision_recall_fscore_support(yb, pb, average=avg, zero_division=0)[i] for avg in ("macro", "weighted") for i in range(3)]
            want += [balanced_accuracy_score(yb, pb), top_k_accuracy_score(yb, logp[rows[b]], k=k, labels=np.arange(V))]
        assert np.abs(stats[b, :FIXED] - np.array(want)).max() <= 1e-12, (b, stats[b, :FIXED], want)
        assert np.abs(stats[b, FIXED:] - values[rows[b]].mean(axis=0)).max() <= 1e-15
        assert np.array_equal(counts[b, :V], np.bincount(yb, minlength=V)) and np.array_equal(counts[b, V:2 * V], np.bincount(pb, minlength=V))
        lost += int(((np.bincount(y, minlength=V) > 0) & (counts[b, :V] == 0)).sum())
    assert lost > 0, "the resamples lose classes"
    assert stats[:, 0].std() > 0 and np.ptp(stats[:, 3]) > 0.0


def test_the_rules_of_a_replicate_on_handmade_rows():
    from slnlp import metrics
    # classes 0..3; class 2 occurs in the predictions only, class 3 nowhere; one label and one prediction are no class
    y = np.array([0, 0, 1, 1, 1, -1, 0])
    pred = np.array([0, 2, 1, 1, 0, 1, 9])
    rank = np.array([0, 1, 0, 0, 2, 0, 1])
    got, counts = replicate_scores(y, pred, rank, 4, 2)
    assert counts.tolist() == [3, 3, 0, 0, 2, 3, 1, 0, 1, 2, 0, 0, 1] and np.array_equal(counts, recount(y, pred, 4))
    p, r = np.array([1 / 2, 2 / 3, 0.0]), np.array([1 / 3, 2 / 3, 0.0])          # over the three classes present
    f = np.array([2 / 5, 4 / 6, 0.0])
    w = np.array([3, 3, 0]) / 6
    want = [3 / 7, p.mean(), r.mean(), f.mean(), (p * w).sum(), (r * w).sum(), (f * w).sum(), (1 / 3 + 2 / 3) / 2, 5 / 7]
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-15, (got, want)      # (row 5 has rank 0 but no class: no hit)
    # the same value outside the classes on both sides is no correct row (the header's accuracy: sum tp_sum / N)
    again, counts2 = replicate_scores(np.append(y, 9), np.append(pred, 9), np.append(rank, 0), 4, 2)
    assert again[0] == 3 / 8 and again[8] == 5 / 8 and counts2[-1] == 2 and counts2[:12].tolist() == counts[:12].tolist()
    assert column_names(0)[-1] is None and np.isnan(replicate_scores(y, pred, None, 4, 0)[0][-1])
    assert column_names(5) == [*metrics.BOOT_COLUMNS[:8], "top5_accuracy"]


def test_the_draw_is_a_function_of_seed_replicate_draw_and_rows():
    a = draws(257, 7, SEED)
    assert a.shape == (7, 257) and a.dtype == np.int64 and a.min() >= 0 and a.max() < 257
    assert np.array_equal(draws(257, 3, SEED), a[:3])                            # replicate b does not depend on B
    assert not np.array_equal(draws(257, 7, SEED + 1), a) and not np.array_equal(draws(257, 7, SEED + (1 << 32)), a)
    assert not np.array_equal(a[0], a[1])
    # draw j is word j & 3 of call j >> 2: the words of the first call, restated from the generator itself
    from threefry_ref import threefry4x32
    u = lambda v: np.array([v], dtype=np.uint32)
    X = threefry4x32([u(0), u(2), u(STAGE), u(0)], [u(SEED & 0xFFFFFFFF), u(SEED >> 32), u(0), u(0)], 12)
    assert [int(x[0]) * 257 >> 32 for x in X] == a[2, :4].tolist()
    assert STAGE not in (0, 1, 2)                                                # the stage words of the class-balanced draw


def test_every_row_is_drawn_about_equally_often():
    """N = 10, B = 2000: a row's total multiplicity is Binomial(B N, 1 / N); within 5 standard deviations of B."""
    N, B = 10, 2000
    total = np.bincount(draws(N, B, SEED).reshape(-1), minlength=N)
    sd = np.sqrt(B * N * (1 / N) * (1 - 1 / N))
    print("multiplicities", total.tolist(), "sd", sd)
    assert total.sum() == B * N and np.abs(total - B).max() <= 5 * sd


def test_the_bootstrap_standard_deviation_of_accuracy():
    """N = 800 at about 0.7 accuracy, B = 2000: within 10 % of sqrt(p (1 - p) / N); the estimate's own relative error is about
    1 / sqrt(2 B) = 1.6 %, so 10 % is six of those."""
    from slnlp import metrics
    N, B = 800, 2000
    y, pred, _, _ = make_case(N, 12, seed=5, hit=0.68)
    p = float((pred == y).mean())
    assert 0.65 <= p <= 0.75
    correct = (pred == y)[draws(N, B, SEED)]                 # accuracy alone: the mean of the gathered hits
    acc = correct.mean(axis=1)
    some = bootstrap_ref(y, pred, None, None, 12, 0, 5, SEED)[0][:, 0]
    assert some.tobytes() == acc[:5].tobytes()               # ... which is the restatement's column
    got = metrics.bootstrap_intervals(acc[:, None], ["accuracy"])["accuracy"]
    want = np.sqrt(p * (1 - p) / N)
    print(f"p {p:.4f}: bootstrap std {got['std']:.5f}, binomial {want:.5f}, ratio {got['std'] / want:.4f}; mean {got['mean']:.4f}")
    assert abs(got["std"] / want - 1.0) <= 0.10
    assert abs(got["mean"] - p) <= 3 * want / np.sqrt(B) * 3 and got["lower"] < p < got["upper"]


# ---------------------------------------------------------------------------------------------------- summarisers ----
def test_intervals_against_np_quantile():
    from slnlp import metrics
    rs = np.random.RandomState(3)
    stats = rs.randn(500, 3) * [1.0, 0.1, 5.0] + [0.0, 0.7, -2.0]
    stats[::7, 2] = np.nan
    for level in (0.95, 0.5, 0.99):
        got = metrics.bootstrap_intervals(stats, ["a", "b", "c"], level=level)
        assert list(got) == ["a", "b", "c"]
        for i, name in enumerate(got):
            x = stats[:, i][~np.isnan(stats[:, i])]
            lo, hi = np.quantile(x, [(1 - level) / 2, 1 - (1 - level) / 2])
            assert got[name] == {"mean": float(x.mean()), "std": float(x.std(ddof=1)), "lower": float(lo), "upper": float(hi),
                                 "n_nan": 500 - x.size}, name
        assert got["c"]["n_nan"] == 72 and got["a"]["n_nan"] == 0 and got["a"]["lower"] < got["a"]["mean"] < got["a"]["upper"]
    empty = metrics.bootstrap_intervals(np.full((4, 1), np.nan), ["x"])["x"]
    assert empty["n_nan"] == 4 and all(np.isnan(empty[k]) for k in ("mean", "std", "lower", "upper"))
    one = metrics.bootstrap_intervals([[0.25]], ["x"])["x"]
    assert (one["mean"], one["lower"], one["upper"], one["n_nan"]) == (0.25, 0.25, 0.25, 0) and np.isnan(one["std"])
    for bad in (0, 1, 1.5, -0.1, True, "0.9", None):
        with pytest.raises(ValueError, match="bootstrap_intervals: level="):
            metrics.bootstrap_intervals(stats, ["a", "b", "c"], level=bad)
    for bad, names in ((stats, ["a", "b"]), (stats[:, 0], ["a"]), (np.zeros((0, 1)), ["a"])):
        with pytest.raises(ValueError, match="bootstrap_intervals: expected"):
            metrics.bootstrap_intervals(bad, names)


def test_difference_against_np_quantile():
    from slnlp import metrics
    rs = np.random.RandomState(4)
    a = rs.randn(400, 2) * 0.05 + [0.72, 0.5]
    b = a - rs.randn(400, 2) * 0.01 - [0.03, 0.0]
    b[5, 1] = np.nan
    a[9, 1] = np.nan
    got = metrics.bootstrap_difference(a, b, ["accuracy", "f1_macro"], level=0.9)
    for i, name in enumerate(("accuracy", "f1_macro")):
        d = a[:, i] - b[:, i]
        d = d[~np.isnan(d)]
        alpha = 1.0 - 0.9
        lo, hi = np.quantile(d, [alpha / 2, 1 - alpha / 2])
        assert got[name] == {"mean": float(d.mean()), "std": float(d.std(ddof=1)), "lower": float(lo), "upper": float(hi),
                             "n_nan": 400 - d.size, "p_not_better": float(np.mean(d <= 0))}, name
    assert got["accuracy"]["p_not_better"] < 0.01 < 0.3 < got["f1_macro"]["p_not_better"] and got["f1_macro"]["n_nan"] == 2
    same = metrics.bootstrap_difference(a[:, :1], a[:, :1], ["accuracy"])["accuracy"]
    assert same == {"mean": 0.0, "std": 0.0, "lower": 0.0, "upper": 0.0, "n_nan": 0, "p_not_better": 1.0}
    with pytest.raises(ValueError, match="bootstrap_difference: the two sets of replicates differ in shape"):
        metrics.bootstrap_difference(a, b[:399], ["accuracy", "f1_macro"])
    with pytest.raises(ValueError, match="bootstrap_difference: expected"):
        metrics.bootstrap_difference(a, b[:, :1], ["accuracy", "f1_macro"])
    with pytest.raises(ValueError, match="bootstrap_difference: level="):
        metrics.bootstrap_difference(a, b, ["accuracy", "f1_macro"], level=1.0)


def test_where_a_name_is_found():
    from slnlp import _lib, metrics
    assert len(metrics.BOOT_COLUMNS) == _lib.BOOT_FIXED == FIXED and metrics.BOOT_COLUMNS[0] == "accuracy"
    assert metrics.BOOT_COLUMNS[-1] == "top_k_accuracy" and len(metrics.BOOT_VALUES) == 3
    assert [metrics.bootstrap_metric_of(n) for n in metrics.BOOT_COLUMNS[:8]] == [(i, 1.0, None) for i in range(8)]
    assert metrics.bootstrap_metric_of("top_k_accuracy") == (8, 1.0, 2) and metrics.bootstrap_metric_of("top5_accuracy") == (8, 1.0, 5)
    assert metrics.bootstrap_metric_of("confidence") == (9, 1.0, None) and metrics.bootstrap_metric_of("neg_brier") == (10, -1.0, None)
    assert metrics.bootstrap_metric_of("neg_log_loss") == (11, -1.0, None)
    for name in ("neg_ece", "neg_ece20", "neg_mce", "roc_auc", "", None):
        assert metrics.bootstrap_metric_of(name) is None, name
    assert all(metrics.is_reduced(n) for n in metrics.BOOT_COLUMNS)


# -------------------------------------------------------------------------------------------------------- options ----
def test_estimator_surface_without_a_gpu():
    from slnlp.net import NeuralNetClassifier
    net = NeuralNetClassifier(module="model.Transformer")
    for call in (net.score_interval, lambda X: net.compare(net, X)):
        with pytest.raises(RuntimeError, match="initialized"):
            call(None)
    # the options are looked at before anything runs: a fitted estimator's surface, without a module
    net.initialized_, net.classes_ = True, np.arange(6)
    for replicates in (0, 65537, 2.5, True, None, "10"):
        with pytest.raises(ValueError, match="score_interval: replicates="):
            net.score_interval(None, replicates=replicates)
    for level in (0, 1, 1.2, True, None, "0.9"):
        with pytest.raises(ValueError, match="score_interval: level="):
            net.score_interval(None, level=level)
    for seed in (-1, 2 ** 64, 0.5, True, None):
        with pytest.raises(ValueError, match="score_interval: seed="):
            net.score_interval(None, seed=seed)
    for scoring in ("neg_ece", "neg_mce", "neg_ece20", ["accuracy", "neg_ece"]):
        with pytest.raises(ValueError, match="has no bootstrap interval here: ECE and MCE"):
            net.score_interval(None, scoring=scoring)
    for scoring in ("roc_auc", ["accuracy", "f2_macro"]):
        with pytest.raises(ValueError, match="has no bootstrap interval; known"):
            net.score_interval(None, scoring=scoring)
    for scoring in ([], ["accuracy", "accuracy"], [3], 3):
        with pytest.raises((ValueError, TypeError), match="scoring"):
            net.score_interval(None, scoring=scoring)
    with pytest.raises(ValueError, match="one call resamples one k"):
        net.score_interval(None, scoring=["top_k_accuracy", "top3_accuracy"])
    with pytest.raises(ValueError, match=r"top6_accuracy: k=6 must lie in \[1, 6\)"):
        net.score_interval(None, scoring="top6_accuracy")
    with pytest.raises(ValueError, match="compare: replicates="):
        net.compare(net, None, replicates=0)
    other = NeuralNetClassifier(module="model.Transformer")
    other.initialized_, other.classes_ = True, np.arange(7)
    with pytest.raises(ValueError, match="compare: the two fits have different classes_"):
        net.compare(other, None)
    assert net._interval_request("score_interval", None, 10, 0.9, 1) == (
        ["accuracy", "precision_macro", "recall_macro", "f1_macro", "precision_weighted", "recall_weighted", "f1_weighted",
         "balanced_accuracy", "top_k_accuracy", "confidence", "neg_brier", "neg_log_loss"], 2, 10, 0.9, 1)
    net.classes_ = np.arange(2)                              # two classes: no top-2 accuracy to resample
    assert "top_k_accuracy" not in net._interval_request("score_interval", None, 10, 0.9, 1)[0]
    assert net._interval_request("score_interval", "top1_accuracy", 10, 0.9, 1)[:2] == (["top1_accuracy"], 1)
    net.classes_ = np.arange(4097)
    with pytest.raises(ValueError, match="score_interval: 4097 classes"):
        net.score_interval(None)
    assert "unclipped" in NeuralNetClassifier.score_interval.__doc__.lower()      # which log-loss this is


def test_cli_key():
    from slnlp import _lib, cli
    assert "confidence_intervals" in cli.DICT_ARGS
    assert cli.confidence_interval_options(None) is None
    assert cli.confidence_interval_options({}) == {"replicates": 1000, "level": 0.95, "seed": 0} == cli.INTERVAL_DEFAULTS
    assert cli.confidence_interval_options({"level": 0.9, "seed": 7}) == {"replicates": 1000, "level": 0.9, "seed": 7}
    assert cli.INTERVAL_MAX_REPLICATES == _lib.BOOT_MAX_REPLICATES
    for bad in ("yes", 5, ["level"], {"levels": 0.9}, {"replicates": 0}, {"replicates": 1}, {"replicates": 65537}, {"replicates": 10.0}, {"replicates": True},
                {"level": 0}, {"level": 1}, {"level": "0.9"}, {"level": True}, {"seed": -1}, {"seed": 2 ** 64}, {"seed": 1.5}):
        with pytest.raises(ValueError, match="confidence_intervals"):
            cli.confidence_interval_options(bad)

    class _Vocab:
        stoi = {"<pad>": 1}

    class _Data:
        vocab_X = vocab_y = _Vocab()
    args = {"model": "model.Transformer", "confidence_intervals": {"replicates": 10}}
    assert "confidence_intervals" not in cli.build_net_params(args, _Data(), "cuda")      # the estimator's options are what they were
    import glob
    for f in glob.glob(os.path.join(ROOT, "tests", "golden", "reference_configs", "config-*.yaml")):
        assert cli.load_config(f).get("confidence_intervals") is None, f

    # a bad key fails before the grid search starts: run() looks at it before it touches the dataset (or needs a device)
    import inspect
    src = inspect.getsource(cli.run)
    assert src.index("confidence_interval_options(") < src.index("load_dataset(") < src.index("gs.fit(")

    # the writer: one score_interval call per k, every name of the run that has an interval, nothing else
    class _Est:
        classes_ = np.arange(5)
        calls = []

        def score_interval(self, data, scoring, **opts):
            self.calls.append((list(scoring), opts))
            return {n: {"point": 0.5, "mean": 0.5, "std": 0.1, "lower": 0.25, "upper": 0.75, "n_nan": 0} for n in scoring}
    import json
    import tempfile
    opts = cli.confidence_interval_options({"replicates": 20})
    with tempfile.TemporaryDirectory() as work:
        out = cli.save_intervals(_Est(), [0] * 24, opts, ["accuracy", "neg_log_loss", "neg_ece", "top3_accuracy", "neg_brier", "top_k_accuracy",
                                                          "top7_accuracy", "roc_auc", "accuracy"], work)
        assert json.load(open(os.path.join(work, "test_intervals.json"))) == out
    assert _Est.calls == [(["accuracy", "neg_log_loss", "neg_brier", "top_k_accuracy"], opts), (["top3_accuracy"], opts)]
    assert sorted(out["intervals"]) == sorted(f"test_{n}" for n in ("accuracy", "neg_log_loss", "neg_brier", "top_k_accuracy", "top3_accuracy"))
    assert (out["replicates"], out["level"], out["seed"], out["rows"]) == (20, 0.95, 0, 24)


def test_buffers_are_slices_of_one_allocation():
    import torch
    from slnlp import ops
    for B, V, Q in ((1, 2, 0), (3, 3, 3), (7, 70, 3), (64, 202, 8)):
        stats, counts = ops.bootstrap_buffers(B, V, Q, True, "cpu")
        assert stats.shape == (B, 9 + Q) and stats.dtype == torch.float64 and counts.shape == (B, 3 * V + 1) and counts.dtype == torch.int32
        assert counts.data_ptr() == stats.data_ptr() + 8 * stats.numel() and stats.untyped_storage().data_ptr() == counts.untyped_storage().data_ptr()
        stats.fill_(1.5)
        counts.copy_(torch.arange(counts.numel(), dtype=torch.int32).view_as(counts))
        h_stats, h_counts = ops.bootstrap_download((stats, counts))
        assert (h_stats == 1.5).all() and h_counts.reshape(-1).tolist() == list(range(counts.numel())) and h_counts.dtype == np.int32
        lean = ops.bootstrap_buffers(B, V, Q, False, "cpu")
        assert lean[1] is None and lean[0].shape == (B, 9 + Q) and ops.bootstrap_download(lean)[1] is None
    apart = (torch.zeros(2, 9, dtype=torch.float64), torch.ones(2, 7, dtype=torch.int32))          # two allocations: two copies
    assert ops.bootstrap_download(apart)[1].tolist() == [[1] * 7] * 2
    for N, V, B in ((1, 2, 1), (5, 3, 3), (257, 70, 7), (800, 202, 1000)):
        buf = ops.score_interval_buffers(N, V, B, "cpu")
        flat = buf["flat"]
        rows, table = buf["reliability"]
        assert flat.dtype == torch.float64 and buf["boot"][0].shape == (B, 12) and buf["boot"][1] is None
        assert rows.shape == (N, 4) and table.shape == (16, 4) and rows.data_ptr() % 32 == flat.data_ptr() % 32 == table.data_ptr() % 32
        pred, picked, rank, counts = buf["score"]
        assert (pred.numel(), picked.numel(), rank.numel(), counts.numel()) == (N, N, N, 3 * V + 1) and picked.dtype == torch.float32
        spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in (buf["boot"][0], table, pred, picked, rank, counts, rows))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[0][0] == flat.data_ptr()
        assert spans[-1] == (rows.data_ptr(), flat.data_ptr() + 8 * flat.numel())               # the rows come last: they stay on the device
        assert flat.data_ptr() + 8 * buf["head"] >= spans[-2][1] and flat.data_ptr() + 8 * buf["head"] <= rows.data_ptr()
    for bad in ((0, 3, 1), (5, 4097, 1), (5, 3, 0), (5, 3, 65537)):
        with pytest.raises(ValueError, match="score_interval_buffers"):
            ops.score_interval_buffers(*bad, "cpu")


# ----------------------------------------------------------------------------------------------------------- C ABI ----
def test_the_entry_point_is_declared_and_bound():
    from slnlp import _lib, ops
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    text = src[src.index("bootstrap of the scores"):src.index("slnlp_bootstrap_scores(")]
    for said in ("(q, b, SLNLP_BOOT_STAGE, 0)", "q = j >> 2", "w = j & 3", "(X_w * N) >> 32", "does not depend on B", "true_sum + pred_sum > 0",
                 "zero_division = 0"):
        assert said in text, f"the header states the draw and the rules so that a caller can restate them: {said!r}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                  # the way tests/test_abi.py reads the header
    assert "slnlp_bootstrap_scores" in set(re.findall(r"\b(slnlp_[a-z0-9_]+)\s*\(", src))
    assert len(_lib.SIGNATURES["slnlp_bootstrap_scores"][1]) == 14
    for macro, value, mirror in (("SLNLP_BOOT_MAX_REPLICATES", 65536, _lib.BOOT_MAX_REPLICATES), ("SLNLP_BOOT_MAX_VALUES", 8, _lib.BOOT_MAX_VALUES),
                                 ("SLNLP_BOOT_FIXED", 9, _lib.BOOT_FIXED)):
        (found,), = [re.findall(rf"#define {macro} (\d+)", src)]
        assert int(found) == value == mirror, macro
    (stage,), = [re.findall(r"#define SLNLP_BOOT_STAGE (0x[0-9a-f]+)u", src)]
    assert int(stage, 16) == _lib.BOOT_STAGE == STAGE and STAGE not in (0, 1, 2)
    common = open(os.path.join(ROOT, "sign-language-nlp_amd", "csrc", "common.hpp")).read()
    assert "SEED_STAGE_BOOTSTRAP = SLNLP_BOOT_STAGE" in common
    for fn in ("bootstrap_scores", "bootstrap_download", "bootstrap_buffers", "score_interval_rows"):
        assert callable(getattr(ops, fn)), fn
    hip = re.sub(r"//.*", "", open(os.path.join(ROOT, "sign-language-nlp_amd", "csrc", "bootstrap.hip")).read())
    assert "SLNLP_ZKERNEL" in hip and "zlaunch" in hip and "SLNLP_CHECK_ARG" in hip and "hipMalloc" not in hip
    assert "SEED_STAGE_BOOTSTRAP" in hip and "seed_words(" in hip
    # integer LDS atomics only: every atomicAdd targets the block's own class counts or tallies
    assert not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", hip)
    assert set(re.findall(r"atomicAdd\(&(\w+)\[", hip)) == {"cls", "tally"} and "atomicAdd(&counts" not in hip and "atomicAdd(&stats" not in hip
    assert "csrc/bootstrap.hip" in open(os.path.join(ROOT, "sign-language-nlp_amd", "Makefile")).read()


def test_the_library_exports_it_and_checks_its_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    lib = _lib.load()
    assert lib.slnlp_abi_version() == 1
    # every check comes before the launch, so a machine without a GPU can ask for the codes and messages (the pointers are
    # never read: they are numbers here)
    good = [64, 128, 256, 512, 4, 3, 5, 3, 2, 4, 7, 1024, 2048]
    for i, value, text in ((0, None, "null pointer"), (11, None, "null pointer"), (2, None, "null pointer"), (6, 0, "N=0 outside"),
                           (7, 4097, "V=4097 outside 1..4096"), (9, 65537, "B=65537 outside 1..65536"), (5, 9, "Q=9 outside 0..8"),
                           (4, 2, "ldv=2 is less than Q=3"), (8, 3, "top_k=3 outside [1, 3)"), (8, -2, "top_k=-2"), (3, 516, "misaligned"),
                           (12, 1030, "misaligned"), (11, 260, "misaligned"), (11, 128, "output stats overlaps input pred"),
                           (12, 64, "output counts overlaps input y"), (12, 1024, "outputs stats and counts overlap")):
        args = list(good)
        args[i] = value
        assert lib.slnlp_bootstrap_scores(*args, None) == 1, (i, value)
        msg = lib.slnlp_last_error().decode()
        assert "bootstrap_scores" in msg and text in msg, (i, value, msg)
