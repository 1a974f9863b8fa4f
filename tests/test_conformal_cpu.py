"""CPU: the numpy restatement of the conformal kernels (tests/conformal_ref.py) against a direct computation, its per-row u
against the generator restatement, the threshold by hand, the coverage guarantee of split conformal prediction on the
restatement, and the host pieces: ``metrics.conformal_report``, the ``conformal`` option, the CLI key, the buffers."""
import csv
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import conformal_ref as cr
from threefry_ref import threefry4x32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-12


def _direct(z, beta, method, lam, k_reg, u):
    """Scores and ranks of every class, row by row: a stable argsort on -value (ties keep ascending columns), then a cumsum."""
    N, V = z.shape
    S, rank = np.empty((N, V)), np.empty((N, V), dtype=np.int64)
    for i in range(N):
        x = z[i].astype(np.float64)
        e = np.exp(beta * x - np.max(beta * x))
        p = e / e.sum()
        order = np.argsort(-x, kind="stable")
        rank[i, order] = np.arange(1, V + 1)
        if method == "lac":
            S[i] = 1.0 - p
            continue
        cum = np.cumsum(p[order])
        for m, c in enumerate(order):
            S[i, c] = (cum[m - 1] if m else 0.0) + u[i] * p[c] + lam * max(0, m + 1 - k_reg)
    return S, rank


@pytest.mark.parametrize("quantum", [None, 0.25])
@pytest.mark.parametrize("beta", [1.0, 0.5])
def test_restatement_against_a_direct_computation(quantum, beta):
    z, y = cr.make_logp(60, 37, 4, quantum=quantum)
    z[3, 5] = -np.inf
    z[7, 1], z[7, 2] = 0.0, -0.0                                                 # equal values: by ascending column
    for method, lam, k_reg, randomized in (("lac", 0.0, 0, False), ("aps", 0.0, 0, False), ("aps", 0.0, 0, True), ("aps", 0.01, 2, True)):
        u = cr.row_u(60, 9, 1) if randomized else np.ones(60)
        want, rank = _direct(z, beta, method, lam, k_reg, u)
        S, got_rank, bad = cr.class_scores(z, beta=beta, method=method, lam=lam, k_reg=k_reg, randomized=randomized, seed=9, draw=1)
        assert not bad.any() and np.array_equal(got_rank, rank)
        assert np.max(np.abs(S - want)) <= BOUND, (method, lam, randomized)
        res = cr.rows_ref(z, y, qhat=0.7, beta=beta, method=method, lam=lam, k_reg=k_reg, randomized=randomized, seed=9, draw=1)
        assert np.array_equal(res["rows"][:, 1], rank[np.arange(60), y]) and np.array_equal(res["mask"], S <= 0.7)
        assert np.array_equal(res["rows"][:, 0], (S <= 0.7).sum(axis=1)) and np.array_equal(res["rows"][:, 2], (S <= 0.7)[np.arange(60), y])
        words = cr.pack_sets(res["mask"])
        assert words.shape == (60, 2) and all(bool(words[i, c >> 5] >> (c & 31) & 1) == res["mask"][i, c] for i in (0, 7, 59) for c in range(37))
        assert (words[:, 1] >> 5 == 0).all()                                     # the padding bits
    assert rank[7, 1] + 1 == rank[7, 2]


def test_codes_of_the_restatement():
    z, y = cr.make_logp(8, 5, 1)
    z[1, 2], z[2, 0] = np.nan, np.inf
    y[3], y[4], y[1] = -1, 5, 9
    res = cr.rows_ref(z, y, qhat=0.5, method="aps")
    assert res["rows"][:, 3].tolist() == [0, -2, -2, -1, -1, 0, 0, 0]             # a NaN row is looked at first
    assert np.isnan(res["score"][[1, 2, 3, 4]]).all() and not np.isnan(res["score"][[0, 5, 6, 7]]).any()
    assert res["rows"][1].tolist() == [0, 0, 0, -2] and not res["mask"][1].any() and res["rows"][3, 0] == res["mask"][3].sum()
    assert cr.rows_ref(z, None, method="lac")["rows"][:, 3].tolist() == [0, -2, -2, 0, 0, 0, 0, 0]


def test_u_is_word_zero_of_the_generator_restatement():
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    stage = int(re.search(r"#define SLNLP_CONFORMAL_STAGE (0x[0-9a-fA-F]+)u", src).group(1), 16)
    boot = int(re.search(r"#define SLNLP_BOOT_STAGE (0x[0-9a-fA-F]+)u", src).group(1), 16)
    from slnlp import _lib
    assert stage == cr.STAGE == _lib.CONFORMAL_STAGE and stage != boot and stage > 2 ** 16      # no stage of the balanced order, no timestep
    for seed, draw in ((0, 0), (0, 1), (12345678901234567890, 7)):
        u = cr.row_u(70, seed, draw)
        for row in (0, 1, 63, 69):
            one = lambda v: np.array([v], dtype=np.uint32)
            w = threefry4x32([one(row), one(draw), one(stage), one(0)], [one(seed & 0xFFFFFFFF), one(seed >> 32), one(0), one(0)], 12)[0][0]
            assert u[row] == (float(w) + 0.5) * 2.0 ** -32 and 0.0 < u[row] < 1.0
    assert not np.array_equal(cr.row_u(70, 0, 0), cr.row_u(70, 0, 1))


def test_threshold_by_hand():
    rs = np.random.RandomState(0)
    for n, k, want in ((1, 2, math.inf), (9, 9, 9.0), (19, 18, 18.0), (8, 9, math.inf)):
        score = rs.permutation(np.arange(1.0, n + 1.0))                          # the k-th smallest is k
        assert cr.quantile_ref(score, np.zeros(n, dtype=int), 0.1) == (want, n, k, 0)
    score = np.array([5.0, np.nan, 1.0, np.nan, 3.0])
    assert cr.quantile_ref(score, [0, -2, 0, -1, 0], 0.5) == (3.0, 3, 2, 2)       # k = ceil(4 * 0.5)
    assert cr.quantile_ref(score, [-1, -2, -1, -1, -2], 0.5) == (math.inf, 0, 1, 5)
    from slnlp.net import conformal_least_rows
    assert [conformal_least_rows(a) for a in (0.1, 0.5, 0.05, 0.2)] == [9, 1, 19, 4]


def test_coverage_guarantee_of_the_restatement():
    """Split conformal prediction with randomised APS covers 1 - alpha up to 1 / (n_cal + 1) in expectation; a trial's coverage is
    Beta-distributed with variance about alpha (1 - alpha) / (n_cal + 2), so the mean of 40 trials has sd 0.0024 (plus the test
    sample's, 0.0011) and the bound of 0.01 is about four of them."""
    n_cal, n_test, V, alpha = 500, 2000, 10, 0.1
    cov, cov_det = [], []
    for seed in range(40):
        rs = np.random.RandomState(1000 + seed)
        logits = 2.0 * rs.randn(n_cal + n_test, V)
        z = (logits - np.log(np.exp(logits).sum(axis=1, keepdims=True))).astype(np.float32)
        p = np.exp(z.astype(np.float64))
        y = (rs.rand(len(z), 1) * p.sum(axis=1, keepdims=True) < np.cumsum(p, axis=1)).argmax(axis=1)      # y ~ softmax(z)
        for randomized, into in ((True, cov), (False, cov_det)):
            cal = cr.rows_ref(z[:n_cal], y[:n_cal], method="aps", randomized=randomized, seed=seed, draw=0)
            qhat, n, k, _ = cr.quantile_ref(cal["score"], cal["rows"][:, 3], alpha)
            assert (n, k) == (n_cal, 451)
            test = cr.rows_ref(z[n_cal:], y[n_cal:], qhat=qhat, method="aps", randomized=randomized, seed=seed, draw=1)
            into.append(test["rows"][:, 2].mean())
    mean, mean_det = float(np.mean(cov)), float(np.mean(cov_det))
    print(f"mean test coverage over 40 trials: randomised APS {mean:.5f}, deterministic APS {mean_det:.5f}; "
          f"target {1 - alpha + 0.5 / (n_cal + 1):.5f}")
    assert abs(mean - (1 - alpha + 0.5 / (n_cal + 1))) <= 0.01
    assert mean_det >= mean and mean_det >= 1 - alpha


def test_report_from_a_table():
    from slnlp import metrics
    z, y = cr.make_logp(80, 6, 3)
    y[y == 4] = 0                                                                # a class without rows
    y[5] = 7
    z[9, 0] = np.nan
    res = cr.rows_ref(z, y, qhat=0.9, method="aps")
    table = cr.summary_ref(res["rows"], y, 6)
    ok = res["rows"][:, 3] == 0
    assert table[6, 0] == 2 and table[:6, 0].sum() == ok.sum() == 78 and table[:, 3].sum() == 78
    rep = metrics.conformal_report(table, state=[0.9, 78.0, 71.0, 2.0], min_support=5)
    sizes, covered = res["rows"][ok, 0], res["rows"][ok, 2]
    assert rep["rows"] == 78 and rep["excluded"] == 2 and rep["coverage"] == covered.mean() and rep["mean_size"] == sizes.mean()
    assert rep["median_size"] == np.sort(sizes)[(78 + 1) // 2 - 1] and rep["empty_rate"] == (sizes == 0).mean()
    assert rep["singleton_rate"] == (sizes == 1).mean() and np.array_equal(rep["size_hist"], np.bincount(sizes, minlength=7))
    assert np.isnan(rep["class_coverage"][4]) and np.isnan(rep["class_mean_size"][4]) and rep["support"][4] == 0
    per = [covered[y[ok] == c].mean() for c in range(6) if c != 4]
    assert np.allclose(np.delete(rep["class_coverage"], 4), per, rtol=0, atol=0) and rep["worst_class_coverage"] == min(per)
    assert (rep["qhat"], rep["calibration_rows"], rep["k"]) == (0.9, 78, 71)
    assert np.isnan(metrics.conformal_report(table, min_support=1000)["worst_class_coverage"])
    empty = metrics.conformal_report(np.zeros((4, 4), dtype=np.int64))
    assert empty["rows"] == 0 and np.isnan(empty["coverage"]) and np.isnan(empty["median_size"])
    with pytest.raises(ValueError, match="conformal_report"):
        metrics.conformal_report(np.zeros((4, 3)))
    with pytest.raises(ValueError, match="min_support"):
        metrics.conformal_report(table, min_support=0)


def test_option_validation_and_get_params_round_trip():
    from slnlp.net import CONFORMAL_DEFAULTS, NeuralNetClassifier, conformal_options
    assert conformal_options(None) is None and conformal_options(False) is None and conformal_options({}) == CONFORMAL_DEFAULTS
    assert CONFORMAL_DEFAULTS == {"alpha": 0.1, "method": "aps", "randomized": True, "lam": 0.0, "k_reg": 0, "seed": 0}
    got = conformal_options({"alpha": 0.2, "method": "lac", "randomized": False, "lam": 1, "k_reg": np.int64(3), "seed": 2 ** 64 - 1})
    assert got == {"alpha": 0.2, "method": "lac", "randomized": False, "lam": 1.0, "k_reg": 3, "seed": 2 ** 64 - 1}
    for bad, text in (("aps", "expected a dict"), ({"level": 0.9}, "unknown keys"), ({"alpha": 0.0}, "alpha"), ({"alpha": 1.0}, "alpha"),
                      ({"alpha": True}, "alpha"), ({"alpha": float("nan")}, "alpha"), ({"method": "raps"}, "method"),
                      ({"randomized": 1}, "randomized"), ({"lam": -0.1}, "lam"), ({"lam": float("inf")}, "lam"), ({"k_reg": -1}, "k_reg"),
                      ({"k_reg": 1.5}, "k_reg"), ({"seed": -1}, "seed"), ({"seed": 2 ** 64}, "seed")):
        with pytest.raises(ValueError, match=text):
            conformal_options(bad)
    setting = {"alpha": 0.2, "method": "lac"}
    net = NeuralNetClassifier(module="model.Transformer", conformal=setting)
    assert net.get_params()["conformal"] == setting and net.conformal == setting
    clone = NeuralNetClassifier(**net.get_params())
    assert clone.get_params() == net.get_params()
    assert NeuralNetClassifier(module="model.Transformer").get_params()["conformal"] is None
    assert net.set_params(conformal=None).get_params()["conformal"] is None


def test_estimator_surface_without_a_gpu():
    from slnlp.ensemble import VotingEnsemble
    from slnlp.net import NeuralNetClassifier
    net = NeuralNetClassifier(module="model.Transformer")
    for name in ("conformalize", "predict_set", "coverage"):
        assert callable(getattr(net, name)) and getattr(VotingEnsemble, name) is getattr(NeuralNetClassifier, name)
    for call in (lambda: net.predict_set(None), lambda: net.coverage(None), lambda: net.conformalize(None)):
        with pytest.raises(RuntimeError, match="not initialized"):
            call()
    net.initialized_ = True                                                      # initialised, but no threshold yet
    with pytest.raises(RuntimeError, match="predict_set: this estimator has no threshold yet"):
        net.predict_set(None)
    with pytest.raises(RuntimeError, match="coverage: this estimator has no threshold yet"):
        net.coverage(None)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            NeuralNetClassifier(module="model.Transformer", conformal={}, device="cuda").initialize()


def test_buffers_are_slices_of_one_allocation():
    from slnlp import ops
    for N, V in ((1, 1), (5, 3), (300, 202), (9, 1024)):
        W = (V + 31) // 32
        buf = ops.conformal_buffers(N, V, "cpu")
        base = buf["flat"].data_ptr()
        assert buf["state"].dtype == torch.float64 and tuple(buf["state"].shape) == (4,) and buf["state"].data_ptr() == base
        assert buf["table"].dtype == torch.int64 and tuple(buf["table"].shape) == (V + 1, 4) and buf["table"].data_ptr() == base + 32
        assert buf["score"].dtype == torch.float64 and tuple(buf["score"].shape) == (N,) and buf["score"].data_ptr() == base + 32 * (V + 2)
        assert buf["rows"].dtype == torch.int32 and tuple(buf["rows"].shape) == (N, 4) and (buf["rows"].data_ptr() - base) % 16 == 0
        assert buf["rows"].data_ptr() >= buf["score"].data_ptr() + 8 * N
        assert buf["sets"].dtype == torch.int32 and tuple(buf["sets"].shape) == (N, W) and buf["sets"].data_ptr() == buf["rows"].data_ptr() + 16 * N
        assert buf["sets"].data_ptr() + 4 * N * W <= base + buf["flat"].numel() * 8
        assert ops.conformal_buffers(N, V, "cpu", sets=False)["sets"] is None
    with pytest.raises(ValueError, match="V=1025"):
        ops.conformal_buffers(5, 1025, "cpu")


def test_cli_key_and_writer(tmp_path):
    from slnlp import cli, metrics
    from slnlp.net import conformal_options
    assert "conformal" in cli.DICT_ARGS
    for bad in ("yes", 5, ["x"], {"level": 0.9}, {"alpha": 2}):                  # what cli.run checks the key with, before the grid search
        with pytest.raises(ValueError, match="conformal"):
            conformal_options(bad)
    z, y = cr.make_logp(60, 5, 2)
    y[y == 3] = 1
    res = cr.rows_ref(z, y, qhat=0.85, method="aps")
    want = metrics.conformal_report(cr.summary_ref(res["rows"], y, 5))

    class _Vocab:
        itos = ["a", "b", "c", "d", "e"]

    class _Data:
        vocab_y = _Vocab()

    class _Est:
        classes_ = np.arange(5)

        def coverage(self, data):
            assert isinstance(data, _Data)
            return dict(want, qhat=0.85, calibration_rows=40, k=37, alpha=0.1, classes=self.classes_)
    cli.save_conformal(_Est(), _Data(), str(tmp_path))
    saved = json.load(open(tmp_path / "test_conformal.json"))
    assert set(saved) == set(cli.CONFORMAL_SCALARS) | {"alpha", "qhat", "n", "k"}
    assert saved["coverage"] == want["coverage"] and saved["mean_size"] == want["mean_size"] and saved["median_size"] == want["median_size"]
    assert (saved["qhat"], saved["n"], saved["k"], saved["alpha"], saved["rows"]) == (0.85, 40, 37, 0.1, 60)
    table = list(csv.reader(open(tmp_path / "test_conformal_classes.csv")))
    assert table[0] == ["class", "name", "support", "coverage", "mean_size"] and len(table) == 6
    for c, line in enumerate(table[1:]):
        assert line[:3] == [str(c), _Vocab.itos[c], str(int(want["support"][c]))]
        if c == 3:
            assert line[3:] == ["", ""]
        else:
            assert float(line[3]) == want["class_coverage"][c] and float(line[4]) == want["class_mean_size"][c]
