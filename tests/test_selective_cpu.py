"""CPU: selective prediction's host side -- the numpy restatement (tests/selective_ref.py) against brute force, ``metrics.selective_report``
on the restatement's table, ``metrics.binomial_upper`` (Clopper-Pearson) and ``metrics.guaranteed_threshold`` (the SGR search),
whose guarantee is checked by simulation on a population with a closed-form selective risk; option checking and persistence."""
import json
import math
import warnings

import numpy as np
import pytest
import torch

import selective_ref as sr


def _brute_counts(kappa, rows):
    inc = sr.included(kappa, rows)
    out = np.zeros((len(kappa), 2), dtype=np.int64)
    for i in np.flatnonzero(inc):
        at_least = inc & (kappa >= kappa[i])
        out[i] = at_least.sum(), (at_least & (rows[:, 1] != 0)).sum()
    return out


def _prefix_risk_mean(kappa, wrong):
    """The usual AURC: sort by descending confidence, mean of the prefix risks.  Defined without ties only."""
    order = np.argsort(-kappa, kind="stable")
    w = np.cumsum(wrong[order].astype(np.float64))
    return math.fsum(w / np.arange(1, len(kappa) + 1)) / len(kappa)


def test_aurc_is_the_mean_of_prefix_risks_without_ties():
    for seed, N in [(0, 1), (1, 2), (2, 17), (3, 500)]:
        kappa, rows = sr.make_counts_case(N, seed)
        assert len(np.unique(kappa)) == N
        s = sr.summary_ref(kappa, rows)
        assert np.array_equal(s["counts"], _brute_counts(kappa, rows))
        assert abs(s["aurc"] - _prefix_risk_mean(kappa, rows[:, 1] != 0)) <= 4 * N * 2.0 ** -53


def test_aurc_is_permutation_invariant_with_heavy_ties():
    kappa, rows = sr.make_counts_case(400, 4, levels=4, excluded=0.1, signed=True)   # the levels: -0.5, -0.25, 0, 0.25
    kappa[kappa == 0.0] = np.where(np.arange((kappa == 0.0).sum()) % 2 == 0, 0.0, -0.0)       # -0.0 ties with +0.0
    assert np.signbit(kappa[kappa == 0.0]).any() and not np.signbit(kappa[kappa == 0.0]).all()
    s = sr.summary_ref(kappa, rows)
    assert np.array_equal(s["counts"], _brute_counts(kappa, rows))
    assert s["excluded_labels"] + s["excluded_nan"] + s["n"] == 400 and s["excluded_nan"] > 0 and s["excluded_labels"] > 0
    for seed in range(3):
        p = np.random.RandomState(seed).permutation(400)
        t = sr.summary_ref(kappa[p], rows[p])
        assert t["aurc"] == s["aurc"] and np.array_equal(t["counts"], s["counts"][p])


def test_oracle_aurc_is_brute_force_on_the_oracle_order():
    from slnlp import metrics
    for n, E in [(1, 0), (1, 1), (10, 3), (257, 0), (257, 257), (1000, 120)]:
        kappa = np.arange(n, 0, -1).astype(np.float64)                           # descending: row 0 is the most confident
        rows = np.zeros((n, 4), dtype=np.int32)
        rows[n - E:, 1] = 1                                                      # every wrong row behind every right one
        s = sr.summary_ref(kappa, rows)
        want = _prefix_risk_mean(kappa, rows[:, 1] != 0)
        assert abs(sr.aurc_oracle(n, E) - want) <= 4 * n * 2.0 ** -53 and metrics.aurc_oracle(n, E) == sr.aurc_oracle(n, E)
        table, _ = sr.table_ref(kappa, rows)
        rep = metrics.selective_report(kappa, rows, s["counts"], table)
        assert rep["rows"] == n and rep["errors"] == E and abs(rep["e_aurc"]) <= 4 * n * 2.0 ** -53
    assert math.isnan(metrics.aurc_oracle(0, 0))


def test_level_tables_are_brute_force():
    from slnlp import metrics
    risks, coverages = [0.0, 0.01, 0.05, 0.1, 0.3, 1.0], [0.0, 0.1, 0.5, 0.8, 0.9, 0.999, 1.0]
    for kappa, rows in [sr.make_counts_case(300, 5), sr.make_counts_case(300, 6, levels=8, excluded=0.05),
                        sr.make_counts_case(50, 7, error_rate=0.0), sr.make_counts_case(50, 8, error_rate=1.0)]:
        table, s = sr.table_ref(kappa, rows, risks, coverages)
        curve = sr.curve_ref(kappa, rows)
        n = s["n"]
        rep = metrics.selective_report(kappa, rows, s["counts"], table, risks, coverages)
        for key in ("threshold", "accepted", "wrong", "coverage", "risk"):
            assert np.array_equal(rep["curve"][key], curve[key]), key
        for r, got in zip(risks, rep["coverage_at_risk"]):
            ok = [i for i in range(len(curve["accepted"])) if float(curve["wrong"][i]) <= r * float(curve["accepted"][i])]
            best = max(ok, key=lambda i: curve["accepted"][i]) if ok else None
            assert got["risk"] == r and got["accepted"] == (curve["accepted"][best] if ok else 0)
            if ok:
                assert got["wrong"] == curve["wrong"][best] and got["threshold"] == curve["threshold"][best]
                assert got["coverage"] == got["accepted"] / n and got["selective_risk"] == got["wrong"] / got["accepted"] <= r
            else:
                assert math.isnan(got["threshold"])
        for c, got in zip(coverages, rep["risk_at_coverage"]):
            ok = [i for i in range(len(curve["accepted"])) if curve["accepted"][i] >= math.ceil(c * n)]
            best = min(ok, key=lambda i: curve["accepted"][i])
            assert (got["accepted"], got["wrong"], got["threshold"]) == (curve["accepted"][best], curve["wrong"][best], curve["threshold"][best])
            assert got["achieved_coverage"] >= c and got["risk"] == got["wrong"] / got["accepted"]
        assert rep["aurc"] == s["aurc"] and rep["accuracy"] == 1.0 - s["E"] / n


def test_rows_restatement_scores():
    with np.errstate(divide="ignore"):
        z = np.log(np.array([[0.7, 0.2, 0.1], [0.4, 0.4, 0.2], [1.0, 0.0, 0.0], [0.5, 0.25, 0.25]], dtype=np.float64)).astype(np.float32)
    p = np.exp(z.astype(np.float64))
    p = p / p.sum(axis=1, keepdims=True)
    y = np.array([0, 2, 0, 7])
    got = {s: sr.rows_ref(z, y, score=s, tau=0.45) for s in sr.SCORES}
    assert np.allclose(got["max_prob"]["kappa"], p.max(axis=1), atol=1e-15)
    assert np.allclose(got["margin"]["kappa"], [p[0, 0] - p[0, 1], 0.0, 1.0, p[3, 0] - p[3, 1]], atol=1e-15) and got["margin"]["kappa"][1] == 0.0
    with np.errstate(all="ignore"):
        ent = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(axis=1)
    assert np.allclose(got["neg_entropy"]["kappa"], ent, atol=1e-15)
    assert got["max_prob"]["rows"].tolist() == [[0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, -1]]
    assert sr.rows_ref(np.zeros((1, 1), dtype=np.float32), score="margin")["kappa"][0] == 1.0
    bad = sr.rows_ref(np.array([[0.0, np.nan], [np.inf, 0.0], [-np.inf, -np.inf]], dtype=np.float32), [5, 0, 0], tau=0.0)
    assert np.isnan(bad["kappa"]).all() and bad["rows"].tolist() == [[1, 0, 0, -2], [0, 0, 0, -2], [0, 0, 0, -2]]


# ------------------------------------------------------------------------------------------------ the binomial bound ----
def _bin_cdf(e, k, b):
    return math.fsum(math.comb(k, i) * b ** i * (1.0 - b) ** (k - i) for i in range(e + 1))


def test_binomial_upper_solves_the_cdf_equation():
    from slnlp import metrics
    for k in (1, 2, 7, 40, 200):
        for delta in (0.5, 0.05, 0.001):
            last = 0.0
            for e in sorted({0, 1, k // 3, k - 1} & set(range(k))):
                b = metrics.binomial_upper(e, k, delta)
                assert 0.0 < b < 1.0 and abs(_bin_cdf(e, k, b) - delta) <= 1e-12, (e, k, delta, b)
                assert b > last                                                  # monotone in e
                last = b
            assert abs(metrics.binomial_upper(0, k, delta) - (1.0 - delta ** (1.0 / k))) <= 1e-14
            assert metrics.binomial_upper(k, k, delta) == 1.0 and metrics.binomial_upper(k + 3, k, delta) == 1.0
    for bad in [(-1, 5, 0.1), (0, 0, 0.1), (1.5, 5, 0.1), (1, 5, 0.0), (1, 5, 1.0), (True, 5, 0.1), (1, 5, None)]:
        with pytest.raises(ValueError, match="binomial_upper"):
            metrics.binomial_upper(*bad)


def test_binomial_upper_is_scipys_beta_quantile():
    stats = pytest.importorskip("scipy.stats")
    from slnlp import metrics
    for e, k, delta in [(0, 10, 0.05), (3, 10, 0.05), (9, 10, 0.5), (17, 400, 0.01), (250, 4000, 0.05 / 12), (399, 4000, 0.004)]:
        assert abs(metrics.binomial_upper(e, k, delta) - stats.beta.ppf(1.0 - delta, e + 1, k - e)) <= 1e-10, (e, k, delta)


# ----------------------------------------------------------------------------------------------------- the guarantee ----
def _draw_curve(rs, n):
    """A calibration draw of the population kappa ~ U(0, 1), P(wrong | kappa) = (1 - kappa)^2, as a curve (no ties)."""
    kappa = np.sort(rs.rand(n))[::-1]
    wrong = rs.rand(n) < (1.0 - kappa) ** 2
    acc = np.arange(1, n + 1)
    w = np.cumsum(wrong)
    return {"threshold": kappa, "accepted": acc, "wrong": w, "coverage": acc / n, "risk": w / acc}


def _true_risk(tau):
    """E[(1 - kappa)^2 | kappa >= tau] = (1 - tau)^2 / 3."""
    return (1.0 - tau) ** 2 / 3.0


def test_the_guarantee_holds_in_simulation_and_the_empirical_rule_has_none():
    from slnlp import metrics
    n, target, delta, T = 4000, 0.1, 0.05, 200
    rs = np.random.RandomState(20240)
    violations, coverage, found, empirical_violations = 0, 0.0, 0, 0
    for _ in range(T):
        curve = _draw_curve(rs, n)
        pick = metrics.guaranteed_threshold(curve, target, delta)
        if pick is not None:
            found += 1
            assert pick["rule"] == "sgr" and pick["bound"] <= target and pick["steps"] == 12
            assert pick["threshold"] == curve["threshold"][pick["index"]] and pick["accepted"] == pick["index"] + 1
            violations += _true_risk(pick["threshold"]) > target
            coverage += 1.0 - pick["threshold"]                                  # the true coverage P[kappa >= tau]
        emp = metrics.guaranteed_threshold(curve, target, None)
        assert emp["rule"] == "empirical" and emp["bound"] is None and emp["risk"] <= target
        empirical_violations += _true_risk(emp["threshold"]) > target
    print(f"SGR: {violations} violations of {T}, found {found}, mean coverage {coverage / T:.4f} (ideal {1.0 - (1.0 - math.sqrt(0.3)):.4f}); "
          f"empirical rule: {empirical_violations} violations of {T}")
    assert violations <= delta * T
    assert coverage / T > 0.4                                                    # reject-all cannot pass
    assert empirical_violations > T / 4                                          # the test tells the two rules apart


def test_guaranteed_threshold_edges():
    from slnlp import metrics
    one = {"threshold": np.array([0.9]), "accepted": np.array([50]), "wrong": np.array([0]), "coverage": np.array([1.0]), "risk": np.array([0.0])}
    pick = metrics.guaranteed_threshold(one, 0.1, 0.05)
    assert pick["steps"] == 1 and pick["index"] == 0 and abs(pick["bound"] - (1.0 - 0.05 ** (1 / 50))) <= 1e-14
    assert metrics.guaranteed_threshold(one, 0.01, 0.05) is None                 # 50 clean rows do not show 1 %
    assert metrics.guaranteed_threshold(one, 0.01, None)["accepted"] == 50
    empty = {k: np.array([]) for k in one}
    assert metrics.guaranteed_threshold(empty, 0.1, 0.05) is None and metrics.guaranteed_threshold(empty, 0.1, None) is None
    hopeless = dict(one, wrong=np.array([50]), risk=np.array([1.0]))
    assert metrics.guaranteed_threshold(hopeless, 0.1, 0.05) is None and metrics.guaranteed_threshold(hopeless, 0.1, None) is None
    for bad in [dict(target_risk=0.0), dict(target_risk=1.0), dict(target_risk="0.1"), dict(target_risk=0.1, delta=0.0),
                dict(target_risk=0.1, delta=1.0), dict(target_risk=0.1, delta=True)]:
        with pytest.raises(ValueError, match="guaranteed_threshold"):
            metrics.guaranteed_threshold(one, **bad)


# ------------------------------------------------------------------------------------------- options and persistence ----
def test_cli_key():
    from slnlp import cli
    assert cli.selective_options(None) is None and "selective" in cli.DICT_ARGS
    assert cli.selective_options({}) == {"score": "max_prob", "risks": [0.01, 0.05, 0.1], "coverages": [0.5, 0.8, 0.9, 1.0]}
    assert cli.selective_options({"score": "margin", "risks": [], "coverages": [1]}) == {"score": "margin", "risks": [], "coverages": [1.0]}
    for bad in ["max_prob", {"scores": "margin"}, {"score": "entropy"}, {"risks": 0.1}, {"risks": [1.5]}, {"coverages": [-0.1]},
                {"risks": [0.1] * 9}, {"coverages": [True]}, {"risks": ["0.1"]}]:
        with pytest.raises(ValueError, match="selective"):
            cli.selective_options(bad)


def test_cli_files(tmp_path):
    import csv

    from slnlp import cli, metrics
    kappa, rows = sr.make_counts_case(60, 9, levels=6)
    opts = cli.selective_options({"risks": [0.2], "coverages": [0.5, 1.0]})
    table, s = sr.table_ref(kappa, rows, opts["risks"], opts["coverages"])
    want = metrics.selective_report(kappa, rows, s["counts"], table, opts["risks"], opts["coverages"])

    class _Est:
        def risk_coverage(self, data, score, risks, coverages):
            assert (data, score, risks, coverages) == ("data", "max_prob", [0.2], [0.5, 1.0])
            return dict(want, score=score, temperature=1.25, classes=np.arange(7))
    cli.save_selective(_Est(), "data", opts, str(tmp_path))
    saved = json.load(open(tmp_path / "test_selective.json"))
    assert set(saved) == set(cli.SELECTIVE_SCALARS) | {"score", "temperature", "coverage_at_risk", "risk_at_coverage"}
    assert saved["aurc"] == want["aurc"] and saved["e_aurc"] == want["e_aurc"] and saved["rows"] == 60 and saved["temperature"] == 1.25
    assert saved["coverage_at_risk"] == want["coverage_at_risk"] and saved["risk_at_coverage"] == want["risk_at_coverage"]
    lines = list(csv.reader(open(tmp_path / "test_risk_coverage.csv")))
    assert lines[0] == ["threshold", "accepted", "wrong", "coverage", "risk"] and len(lines) == 1 + len(want["curve"]["threshold"])
    for i, line in enumerate(lines[1:]):
        assert float(line[0]) == want["curve"]["threshold"][i] and int(line[1]) == want["curve"]["accepted"][i]
        assert int(line[2]) == want["curve"]["wrong"][i] and float(line[4]) == want["curve"]["risk"][i]


def test_ops_refuse_bad_levels_before_touching_the_device():
    from slnlp import ops
    assert ops._selective_levels("x", "risks", (0, 0.5, 1)) == [0.0, 0.5, 1.0]
    for bad in [(1.5,), (-0.1,), (float("nan"),), (0.1,) * 9, 0.1, ("a",)]:
        with pytest.raises(ValueError, match="x: risks"):
            ops._selective_levels("x", "risks", bad)


class _Stub:
    """What ``save_params`` / ``load_params`` touch around rejection.json, without a module."""
    initialized_ = True
    _fused = False
    history = []
    calibration_ = None

    class _Module:
        def state_dict(self):
            return {}

        def load_state_dict(self, sd):
            pass

    class _Opt:
        param_groups = [{"lr": 0.1}]

        def state_dict(self):
            return {}

        def load_state_dict(self, sd):
            pass
    _groups = None
    device = "cpu"


def _stub():
    from slnlp.net import NeuralNetClassifier
    cls = type("StubNet", (_Stub, NeuralNetClassifier), {"__init__": lambda self: None})
    net = cls()
    net.module_, net.optimizer_, net.criterion_ = _Stub._Module(), _Stub._Opt(), _Stub._Module()
    return net


def test_rejection_json_round_trip(tmp_path):
    net = _stub()
    with pytest.raises(RuntimeError, match="no rejection threshold yet"):
        net.predict_selective(None)
    for threshold, bound, risk in [(0.1 + 0.2, 0.0481, 0.03), (float("inf"), None, float("nan"))]:
        info = {"score": "margin", "rule": "sgr", "target_risk": 0.05, "delta": 0.05, "threshold": threshold, "bound": bound,
                "accepted": 0 if bound is None else 310, "wrong": 0 if bound is None else 9, "coverage": 0.0 if bound is None else 0.775,
                "risk": risk, "n": 400, "excluded": 2, "calibrated": False}
        net._set_rejection(info)
        assert net._rej_state.dtype == torch.float64 and net._rej_state.tolist()[0] == threshold
        net.save_params(str(tmp_path))
        back = _stub()
        back.load_params(str(tmp_path))
        assert back._rej_state.tolist() == net._rej_state.tolist() and back.rejection_["threshold"] == threshold
        for k, v in info.items():
            assert back.rejection_[k] == v or (k == "risk" and math.isnan(v) and math.isnan(back.rejection_[k])), k
    net._set_rejection(None)
    assert not hasattr(net, "rejection_") and not hasattr(net, "_rej_state")
    net._set_rejection(None)                                                     # twice is fine


def test_estimator_option_checks_come_before_the_forward_pass():
    net = _stub()
    with pytest.raises(ValueError, match="risk_coverage: score"):
        net.risk_coverage(None, score="entropy")
    with pytest.raises(ValueError, match="risk_coverage: risks"):
        net.risk_coverage(None, risks=(2.0,))
    with pytest.raises(ValueError, match="fit_rejection: score"):
        net.fit_rejection(None, score="top1")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        from slnlp.ensemble import VotingEnsemble
        from slnlp.prior_shift import PriorShift
        for cls in (VotingEnsemble, PriorShift):
            assert all(hasattr(cls, m) for m in ("risk_coverage", "fit_rejection", "predict_selective", "_set_rejection"))
