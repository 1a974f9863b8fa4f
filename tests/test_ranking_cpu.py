"""CPU: the ranking metrics' definitions -- the numpy restatement (tests/ranking_ref.py) against sklearn's binary ``roc_auc_score``
and ``average_precision_score`` per class, ``slnlp.metrics``' host side (names, ``ranking_from_table``, ``ranking_numpy``,
``epoch_scores`` on CPU tensors, ``ScoringWrapper``), the estimator's surface without a GPU and the CLI key.

The bound against sklearn is 1e-12: both sides are fp64 sums of at most N terms of size <= 1 at N <= 300, so their rounding is at
most N 2^-52 < 1e-13."""
import csv
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

from ranking_ref import NAMES, make_scores, ranking_ref, rows_ref, summary_ref, table_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-12


def _cases():
    flat, y_flat = make_scores(120, 5, 3)
    flat[:, 2] = np.float32(-1.25)                                              # a column of equal values: AUC 0.5
    return [("random", *make_scores(300, 37, 1)), ("quantised", *make_scores(300, 37, 2, quantum=0.25)),
            ("absent_classes", *make_scores(200, 40, 4, quantum=0.5, absent=(0, 7, 39))), ("flat_column", flat, y_flat)]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_restatement_against_sklearn_per_class(case):
    from sklearn.metrics import average_precision_score, roc_auc_score
    name, z, y = case
    rows, table, got = ranking_ref(z, y)
    V = z.shape[1]
    defined = 0
    for c in range(V):
        P = int((y == c).sum())
        if P == 0 or P == len(y):
            assert np.isnan(got["auc"][c]) and np.isnan(got["ap"][c]), (name, c)
            continue
        defined += 1
        auc, ap = roc_auc_score(y == c, z[:, c]), average_precision_score(y == c, z[:, c])
        assert abs(got["auc"][c] - auc) <= BOUND and abs(got["ap"][c] - ap) <= BOUND, (name, c, got["auc"][c], auc, got["ap"][c], ap)
    assert got["classes_scored"] == defined > 0
    if name == "quantised":                                                     # the ties are there: most rows share their value with a negative
        assert (rows[:, 1] > 0).mean() > 0.9
    if name == "flat_column":
        assert got["auc"][2] == 0.5 and abs(got["ap"][2] - (y == 2).mean()) <= BOUND
    d = ~np.isnan(got["auc"])
    w = got["support"][d]
    assert abs(got["auc_macro"] - got["auc"][d].mean()) <= BOUND and abs(got["ap_weighted"] - (got["ap"][d] * w).sum() / w.sum()) <= BOUND


def test_undefined_classes_are_left_out_where_sklearn_gives_up():
    from sklearn.metrics import roc_auc_score
    from slnlp import metrics
    z, y = make_scores(200, 40, 4, quantum=0.5, absent=(0, 7, 39))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            theirs = roc_auc_score(y, np.exp(z.astype(np.float64)) / np.exp(z.astype(np.float64)).sum(1, keepdims=True), multi_class="ovr",
                                   labels=np.arange(40))
        except ValueError:
            theirs = float("nan")
    assert np.isnan(theirs)
    got = metrics.ranking_from_table(metrics.ranking_numpy(z, y)[1])
    assert got["classes_scored"] == 37 and all(np.isfinite(got[k]) for k in NAMES)
    assert np.isnan(got["auc"][[0, 7, 39]]).all() and np.isnan(got["ap"][[0, 7, 39]]).all() and got["support"][[0, 7, 39]].tolist() == [0, 0, 0]
    # nothing defined: everything NaN
    one = metrics.ranking_from_table(metrics.ranking_numpy(z[:, :1], np.zeros(200, dtype=np.int64))[1])
    assert one["classes_scored"] == 0 and all(np.isnan(one[k]) for k in NAMES)


def test_ranking_numpy_is_the_restatement():
    from slnlp import metrics
    special, ys = make_scores(64, 6, 9, quantum=0.5)
    special[3, 1], special[9, 1], special[10, 1] = -np.inf, -0.0, 0.0
    special[5, 4] = np.nan
    ys[7], ys[8] = -1, 6
    for z, y in [c[1:] for c in _cases()] + [(special, ys)]:
        rows, table, want = ranking_ref(z, y)
        got_rows, got_table = metrics.ranking_numpy(z, y)
        assert got_rows.dtype == np.int32 and np.array_equal(got_rows, rows)
        assert np.array_equal(got_table[:, :3], table[:, :3])
        assert np.allclose(got_table[:, 3], table[:, 3], rtol=300 * 2.0 ** -52, atol=0.0)
        got = metrics.ranking_from_table(got_table)
        for k in NAMES:
            assert abs(got[k] - want[k]) <= BOUND, k
        assert got["classes_scored"] == want["classes_scored"] and np.array_equal(got["support"], want["support"])
        assert np.allclose(got["auc"], want["auc"], rtol=0, atol=BOUND, equal_nan=True)
        assert np.allclose(got["ap"], want["ap"], rtol=0, atol=BOUND, equal_nan=True)
    rows, table, want = ranking_ref(special, ys)
    assert rows[7].tolist() == [0, 0, 0, -1] and rows[8].tolist() == [0, 0, 0, -1] and table[6].tolist() == [62.0, 2.0, 0.0, 0.0]
    assert table[4, 1] == 1 and np.isnan(want["auc"][4]) and (rows[ys == 4, 3] == -2).all() and (rows[ys == 4, :3] == 0).all()
    assert want["classes_scored"] == 5
    got = metrics.ranking_from_table(table)
    assert (got["rows"], got["bad_labels"], got["nan_classes"]) == (62, 2, 1)


def test_names_and_families():
    from slnlp import metrics
    assert metrics.RANKING == NAMES
    assert all(metrics.is_reduced(n) for n in metrics.RANKING)
    assert not metrics.is_reduced("roc_auc_ovr") and not metrics.is_reduced("auc") and not metrics.is_reduced("ap_micro")
    assert all(metrics.bootstrap_metric_of(n) is None for n in metrics.RANKING)
    assert all(metrics.calibration_metric_of(n) is None and metrics.top_k_of(n) is None for n in metrics.RANKING)
    with pytest.raises(ValueError, match="ranking_from_table"):
        metrics.ranking_from_table(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="ranking"):
        metrics.ranking_numpy(np.zeros((3, 2)), np.zeros(4))


def test_epoch_scores_on_cpu_tensors():
    from slnlp import metrics
    z, y = make_scores(257, 12, 5, quantum=0.25, absent=(3,))
    want = ranking_ref(z, y)[2]
    got = metrics.epoch_scores(["accuracy", "auc_macro", "ap_macro", "roc_auc_ovr", "ap_weighted"], torch.from_numpy(z), torch.from_numpy(y))
    assert set(got) == {"accuracy", "auc_macro", "ap_macro", "ap_weighted"}
    for k in ("auc_macro", "ap_macro", "ap_weighted"):
        assert abs(got[k] - want[k]) <= BOUND, k
    assert got["accuracy"] == float((z.argmax(1) == y).mean())
    assert set(metrics.epoch_scores(["auc_weighted"], torch.from_numpy(z), torch.from_numpy(y))) == {"auc_weighted"}
    bad = y.copy()
    bad[4] = 12
    with pytest.raises(ValueError, match="scoring the valid data: 1 of 257 labels lie outside the 12 classes"):
        metrics.epoch_scores(["ap_macro"], torch.from_numpy(z), torch.from_numpy(bad), split="valid")


def test_scoring_wrapper():
    from slnlp.net import ScoringWrapper, _CachedPredictor
    z, y = make_scores(150, 6, 8, quantum=0.25)
    proba = np.exp(z.astype(np.float64))
    want = ranking_ref(proba, y)[2]
    labels = np.arange(6)
    for name in NAMES:
        wr = ScoringWrapper(name, labels)
        assert wr.greater_is_better and wr.score == name and ScoringWrapper.needs_labels(name)
        assert abs(wr(_CachedPredictor(proba, labels), None, y) - want[name]) <= BOUND, name
    # labels that are not the column indices map as in calibration_error
    names = np.array([10, 20, 30, 40, 50, 60])
    assert abs(ScoringWrapper("ap_macro", names)(_CachedPredictor(proba, names), None, names[y]) - want["ap_macro"]) <= BOUND
    with pytest.raises(ValueError, match="auc_macro: 1 of 150 labels lie outside the 6 classes"):
        ScoringWrapper("auc_macro", names)(_CachedPredictor(proba, names), None, np.where(np.arange(150) == 2, 35, names[y]))
    assert not ScoringWrapper.needs_labels("roc_auc_ovr")


def test_two_classes_and_a_one_dimensional_proba():
    from sklearn.metrics import average_precision_score, roc_auc_score
    from slnlp import metrics
    rs = np.random.RandomState(3)
    y = rs.randint(0, 2, size=90)
    p = np.round(np.clip(0.5 + 0.3 * (y - 0.5) + 0.25 * rs.randn(90), 0.01, 0.99), 2)
    auc = metrics.ranking_score(y, p, name="auc_macro")
    assert abs(auc - roc_auc_score(y, p)) <= BOUND                               # both classes have the same one-vs-rest AUC
    ap = metrics.ranking_score(y, p, name="ap_macro", labels=[0, 1])
    assert abs(ap - 0.5 * (average_precision_score(y, p) + average_precision_score(1 - y, 1.0 - p))) <= BOUND
    assert metrics.ranking_score(y, np.stack([1.0 - p, p], axis=1), name="ap_macro") == ap


def test_estimator_surface_without_a_gpu():
    from slnlp.ensemble import VotingEnsemble
    from slnlp.net import NeuralNetClassifier
    net = NeuralNetClassifier(module="model.Transformer")
    assert callable(net.ranking) and VotingEnsemble.ranking is NeuralNetClassifier.ranking
    with pytest.raises(RuntimeError, match="not initialized"):
        net.ranking(None)
    # no bootstrap interval: the existing message
    net.initialized_, net.classes_ = True, np.arange(6)
    for name in NAMES:
        with pytest.raises(ValueError, match="has no bootstrap interval; known"):
            net.score_interval(None, scoring=name)


def test_the_entry_point_is_declared_and_bound():
    from slnlp import _lib
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    block = src[src.index("ranking metrics --"):src.index("int slnlp_ranking_rows(")]
    assert "sklearn" in block and "-0.0" in block and "NaN" in block
    assert f"#define SLNLP_RANK_CHUNK {_lib.RANK_CHUNK}\n" in src and f"#define SLNLP_RANK_MAX_ROWS {_lib.RANK_MAX_ROWS} " in src
    assert 2 * _lib.RANK_MAX_ROWS ** 2 < 2 ** 53 <= 2 * (_lib.RANK_MAX_ROWS + 1) ** 2
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"\bslnlp_ranking_rows\s*\(([^)]*)\)", src)
    assert decl and len(decl.group(1).split(",")) == 8 == len(_lib.SIGNATURES["slnlp_ranking_rows"][1])
    mk = open(os.path.join(ROOT, "sign-language-nlp_amd", "Makefile")).read()
    assert "csrc/ranking.hip" in mk


def test_buffers_are_slices_of_one_allocation():
    from slnlp import ops
    for N, V in ((1, 1), (5, 3), (300, 202)):
        rows, table = ops.ranking_buffers(N, V, "cpu")
        assert rows.dtype == torch.int32 and tuple(rows.shape) == (N, 4) and table.dtype == torch.float64 and tuple(table.shape) == (V + 1, 4)
        assert rows.untyped_storage().data_ptr() == table.untyped_storage().data_ptr() == table.data_ptr()
        assert rows.data_ptr() == table.data_ptr() + 32 * (V + 1) and table.untyped_storage().nbytes() == 32 * (V + 1) + 16 * N
        none, only = ops.ranking_buffers(N, V, "cpu", per_row=False)
        assert none is None and only._base.numel() == 4 * (V + 1)


def test_cli_key_and_writer(tmp_path):
    from slnlp import cli
    assert "ranking" in cli.DICT_ARGS
    assert cli.ranking_options(None) is None and cli.ranking_options({}) == {}
    for bad in ("yes", 5, ["x"], {"average": "macro"}, {1: 2}):
        with pytest.raises(ValueError, match="ranking"):
            cli.ranking_options(bad)
    z, y = make_scores(60, 5, 2, quantum=0.5, absent=(3,))
    want = ranking_ref(z, y)[2]

    class _Vocab:
        itos = ["a", "b", "c", "d", "e"]

    class _Data:
        vocab_y = _Vocab()

    class _Est:
        classes_ = np.arange(5)

        def ranking(self, data):
            assert isinstance(data, _Data)
            return dict(want, classes=self.classes_, temperature=1.0)
    res = cli.save_ranking(_Est(), _Data(), {}, str(tmp_path))
    assert res["classes_scored"] == 4
    saved = json.load(open(tmp_path / "test_ranking.json"))
    assert set(saved) == set(NAMES) | {"classes_scored"} and saved["classes_scored"] == 4
    assert all(saved[k] == want[k] for k in NAMES)
    table = list(csv.reader(open(tmp_path / "test_ranking_classes.csv")))
    assert table[0] == ["class", "name", "support", "auc", "ap"] and len(table) == 6
    for c, line in enumerate(table[1:]):
        assert line[:3] == [str(c), _Vocab.itos[c], str(int(want["support"][c]))]
        if c == 3:
            assert line[3:] == ["", ""]
        else:
            assert float(line[3]) == want["auc"][c] and float(line[4]) == want["ap"][c]
