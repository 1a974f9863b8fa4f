"""CPU: the confident-learning audit without a GPU -- the numpy restatement (tests/label_audit_ref.py) on examples whose answer is
known by hand or by construction, ``metrics.label_audit_report``'s algebra and orders, ``slnlp.OutOfFold``'s constructor, the CLI
key and the estimator method's own checks.  The device is held to the restatement in tests/test_label_audit_gpu.py."""
import math

import numpy as np
import pytest

import label_audit_ref as lr


def _logp(p):
    return np.log(np.asarray(p, dtype=np.float64)).astype(np.float32)


HAND_P = [[0.90, 0.05, 0.05],        # y 0: confidently 0
          [0.70, 0.20, 0.10],        # y 0: below t_0 = 0.8, confidently nothing
          [0.10, 0.80, 0.10],        # y 1: confidently 1
          [0.85, 0.10, 0.05],        # y 1: confidently 0 -- the label issue
          [0.10, 0.20, 0.70],        # y 2: confidently 2
          [0.30, 0.30, 0.40]]        # y 2: confidently nothing; its two other columns tie, the first one counts
HAND_Y = [0, 0, 1, 1, 2, 2]


def test_hand_worked_example():
    """s = (.9, .7, .8, .1, .7, .4), so t = (.8, .45, .55); row 3 alone reaches another class's threshold.  The float32 log-probs
    carry the probabilities to about 1e-8, and nothing here lies closer than 0.05 to a threshold."""
    from slnlp import metrics
    ref = lr.audit_ref(_logp(HAND_P), HAND_Y)
    near = lambda a, b: np.allclose(a, b, rtol=0.0, atol=1e-6)
    assert near(ref["s"], [0.9, 0.7, 0.8, 0.1, 0.7, 0.4]) and near(ref["t"], [0.8, 0.45, 0.55]) and ref["n"].tolist() == [2, 2, 2]
    assert near(ref["other"], [0.05, 0.2, 0.1, 0.85, 0.2, 0.3]) and near(ref["m"], [0.85, 0.5, 0.7, -0.75, 0.5, 0.1])
    assert lr.smallest_gap(ref, HAND_Y) > 0.04
    assert ref["pred"].tolist() == [0, 0, 1, 0, 2, 2] and ref["code"].tolist() == [0] * 6
    assert ref["k"].tolist() == [0, -1, 1, 0, 2, -1] and ref["flags"].tolist() == [0, 0, 0, 3, 0, 0]
    assert ref["joint"].tolist() == [[1, 0, 0], [1, 1, 0], [0, 0, 1]] and ref["overflow"] == 2 and ref["pairs"] == [(1, 0, 1)]
    assert ref["counts"] == {"usable": 6, "bad_labels": 0, "nan_rows": 0, "unconfident": 2, "issues": 1, "argmax_disagrees": 1}
    rep = metrics.label_audit_report(lr.record_of(ref), HAND_Y)
    assert rep["issues"]["row"].tolist() == [3] and rep["issues"]["given"].tolist() == [1] and rep["issues"]["suggested"].tolist() == [0]
    assert near(rep["issues"]["self_confidence"], [0.1]) and near(rep["issues"]["margin"], [-0.75])
    # r = (1, 2, 1) and n = (2, 2, 2): rows scaled to the support, divided by 6
    assert np.array_equal(rep["calibrated_joint"], np.array([[2.0, 0, 0], [1.0, 1.0, 0], [0, 0, 2.0]]) / 6.0)
    assert rep["noise_rate"] == pytest.approx(1.0 / 6.0, abs=1e-15)
    assert rep["per_class"]["noise"].tolist() == [0.0, 0.5, 0.0] and rep["per_class"]["issues"].tolist() == [0, 1, 0]
    assert rep["per_class"]["confident_other"].tolist() == [1, 0, 0] and rep["per_class"]["support"].tolist() == [2, 2, 2]
    assert rep["pairs"] == [(1, 0, 1)] and (rep["rows"], rep["unconfident"], rep["argmax_disagrees"]) == (6, 2, 1)
    assert (rep["bad_labels"], rep["nan_rows"]) == (0, 0)


def _planted(V=5, clean=8, flips=((0, 1), (0, 1), (2, 4), (3, 0), (4, 2), (1, 3))):
    """Per class ``clean`` rows with the true-class probability running over [0.80, 0.95] and the rest uniform; per (true, given) in
    ``flips`` one row with weight 0.95 on the true class, 0.06 on the given one and 1e-9 elsewhere (the softmax normalises the
    1.01: 0.9406 and 0.0594).  Returns (z, given labels, true labels, flipped rows, flip matrix [given][true])."""
    rows, given, true = [], [], []
    for c in range(V):
        for q in np.linspace(0.80, 0.95, clean):
            p = np.full(V, (1.0 - q) / (V - 1))
            p[c] = q
            rows.append(p); given.append(c); true.append(c)
    flipped, F = [], np.zeros((V, V), dtype=np.int64)
    for c, g in flips:
        p = np.full(V, 1e-9)
        p[c], p[g] = 0.95, 0.06
        flipped.append(len(rows))
        rows.append(p); given.append(g); true.append(c)
        F[g, c] += 1
    order = np.random.RandomState(3).permutation(len(rows))              # the flipped rows anywhere among the others
    where = np.empty(len(rows), dtype=np.int64)
    where[order] = np.arange(len(rows))
    return (_logp(rows)[order], np.array(given)[order], np.array(true)[order], np.sort(where[flipped]), F)


def test_planted_noise_is_found_exactly():
    from slnlp import metrics
    z, given, true, flipped, F = _planted()
    ref = lr.audit_ref(z, given)
    assert lr.smallest_gap(ref, given) >= 0.01                                  # the condition that makes the answer exact
    rep = metrics.label_audit_report(lr.record_of(ref), given)
    assert np.array_equal(np.sort(rep["issues"]["row"]), flipped)
    assert np.array_equal(rep["issues"]["suggested"], true[rep["issues"]["row"]])
    assert np.array_equal(rep["issues"]["given"], given[rep["issues"]["row"]])
    off = ref["joint"] - np.diag(np.diagonal(ref["joint"]))
    assert np.array_equal(off, F)
    assert sorted(rep["pairs"]) == sorted((g, c, int(F[g, c])) for g in range(5) for c in range(5) if F[g, c])
    assert rep["pairs"][0] == (1, 0, 2)                                          # the one cell with two rows first
    assert np.array_equal(rep["per_class"]["issues"], F.sum(axis=1)) and np.array_equal(rep["per_class"]["confident_other"], F.sum(axis=0))
    assert rep["argmax_disagrees"] == len(flipped) and rep["noise_rate"] > 0.0
    # a clean row is confidently its own class or nothing, never flagged
    clean = np.setdiff1d(np.arange(len(given)), flipped)
    assert set(ref["k"][clean] - given[clean] * (ref["k"][clean] >= 0)) <= {0, -1} and not ref["flags"][clean].any()


def test_thresholds_of_empty_and_single_row_classes():
    z = _logp([[0.6, 0.3, 0.05, 0.05], [0.5, 0.3, 0.1, 0.1], [0.2, 0.2, 0.5, 0.1]])
    y = [0, 0, 2]
    ref = lr.audit_ref(z, y)
    assert ref["n"].tolist() == [2, 0, 1, 0] and math.isnan(ref["t"][1]) and math.isnan(ref["t"][3])
    assert ref["t"][2] == ref["s"][2]                                            # its own s, bit for bit: equality means confident
    assert ref["k"][2] == 2 and ref["flags"][2] == 0
    assert not (ref["k"] == 1).any() and not (ref["k"] == 3).any()               # a NaN threshold compares false: nobody is confidently 1 or 3
    # excluded rows: the NaN is looked at first, then the label
    z2 = np.vstack([z, _logp([[0.25] * 4]), _logp([[0.25] * 4])])
    z2[3, 1] = np.nan
    ref2 = lr.audit_ref(z2, [0, 0, 2, 9, 7])
    assert ref2["code"].tolist() == [0, 0, 0, -2, -1] and ref2["k"][3:].tolist() == [-1, -1] and ref2["flags"][3:].tolist() == [0, 0]
    assert np.array_equal(ref2["t"][[0, 2]], ref["t"][[0, 2]]) and ref2["overflow"] == ref["overflow"] + 2
    assert ref2["counts"]["nan_rows"] == 1 and ref2["counts"]["bad_labels"] == 1 and ref2["counts"]["usable"] == 3
    one = lr.audit_ref(np.zeros((1, 1), dtype=np.float32), [0])
    assert (one["s"][0], one["other"][0], one["m"][0], one["t"][0], one["k"][0], one["flags"][0]) == (1.0, 0.0, 1.0, 1.0, 0, 0)


def test_report_algebra():
    from slnlp import metrics
    import conformal_ref as cr
    for N, V, seed in [(60, 4, 1), (300, 12, 2), (40, 30, 3)]:                   # the last: classes without rows, single-row classes
        z, y = cr.make_logp(N, V, seed, lean=2.0)
        ref = lr.audit_ref(z, y)
        rep = metrics.label_audit_report(lr.record_of(ref), y)
        q, n = rep["calibrated_joint"], ref["n"]
        assert abs(q.sum() - 1.0) <= 1e-12 and np.abs(q.sum(axis=1) - n / n.sum()).max() <= 1e-12
        assert abs(rep["noise_rate"] - (1.0 - np.trace(q))) <= 1e-15 and 0.0 <= rep["noise_rate"] <= 1.0
        r = ref["joint"].sum(axis=1)
        for c in np.flatnonzero((r == 0) & (n > 0)):                             # no confident row: no evidence of noise
            assert q[c, c] == n[c] / n.sum() and rep["per_class"]["noise"][c] == 0.0
        assert np.isnan(rep["per_class"]["noise"][n == 0]).all() and not np.isnan(rep["per_class"]["noise"][n > 0]).any()
        assert len(rep["issues"]["row"]) == ref["counts"]["issues"] == int(rep["per_class"]["issues"].sum())
        assert rep["joint"].sum() + ref["overflow"] == N


def test_ranking_order_and_ties():
    from slnlp import metrics
    N = 8
    rec = {"head": np.array([N, 0, 0, 0, 6, 6, 0, 0]), "t": np.full(2, 0.5), "n": np.array([4, 4], dtype=np.int32),
           "joint": np.array([[1, 3], [3, 1]]), "overflow": 0, "pairs": np.array([[0, 1, 3], [1, 0, 3], [-1, -1, 0]], dtype=np.int32),
           "k": np.array([1, 1, 1, 0, 0, 0, 0, 1], dtype=np.int32), "code": np.zeros(N, dtype=np.int32),
           "flags": np.array([3, 3, 3, 3, 3, 3, 0, 0], dtype=np.int32),
           "s": np.array([0.30, 0.10, 0.30, 0.20, 0.10, 0.40, 0.9, 0.9]),
           "m": np.array([-0.2, -0.5, -0.2, -0.5, -0.1, -0.2, 0.8, 0.8])}
    y = np.array([0, 0, 0, 1, 1, 1, 0, 1])
    by_m = metrics.label_audit_report(rec, y)
    assert by_m["rank_by"] == "normalized_margin" and by_m["issues"]["row"].tolist() == [1, 3, 0, 2, 5, 4]      # ties by ascending row
    assert by_m["issues"]["margin"].tolist() == [-0.5, -0.5, -0.2, -0.2, -0.2, -0.1]
    by_s = metrics.label_audit_report(rec, y, rank_by="self_confidence")
    assert by_s["issues"]["row"].tolist() == [1, 4, 3, 0, 2, 5] and by_s["issues"]["suggested"].tolist() == [1, 0, 0, 1, 1, 0]
    assert by_s["pairs"] == [(0, 1, 3), (1, 0, 3)]
    with pytest.raises(ValueError, match="rank_by='entropy'"):
        metrics.label_audit_report(rec, y, rank_by="entropy")
    with pytest.raises(ValueError, match="label_audit_report: y has shape"):
        metrics.label_audit_report(rec, y[:-1])


def test_out_of_fold_constructor_refusals():
    import slnlp
    from slnlp.net import NeuralNetClassifier
    from slnlp.out_of_fold import OutOfFold, check_partition, cross_fit
    assert slnlp.OutOfFold is OutOfFold and slnlp.cross_fit is cross_fit and {"OutOfFold", "cross_fit"} <= set(slnlp.__all__)
    assert OutOfFold.label_issues is NeuralNetClassifier.label_issues and OutOfFold.reliability is NeuralNetClassifier.reliability

    def fitted(n_classes, device="cuda:0"):
        net = NeuralNetClassifier(module="model.Transformer", device=device)
        net.initialized_, net.classes_ = True, np.arange(n_classes)
        return net
    a, b = fitted(6), fitted(6)
    folds = [np.array([0, 2, 4]), np.array([1, 3])]
    oof = OutOfFold([a, b], folds)
    assert oof.calibration_ is None and oof.temperature_ == 1.0 and oof.initialized_ and oof.rows_ == 5 and oof.calibrated
    assert oof.members == [a, b] and np.array_equal(oof.classes_, np.arange(6)) and all(f.dtype == np.int64 for f in oof.folds)
    ens = oof.ensemble(voting="log")
    assert type(ens).__name__ == "VotingEnsemble" and ens.members == [a, b] and ens.voting == "log"
    for bad in ([[0, 1], [1, 2]], [[0, 1], [3, 4]], [[0, 1], [2, 5]], [[0, 1], []], [[-1, 0], [1, 2]], [[0, 1], [[2]]]):
        with pytest.raises(ValueError, match="OutOfFold: (the folds must partition|folds must be a list)"):
            OutOfFold([a, b], bad)
    with pytest.raises(ValueError, match="2 members and 3 folds"):
        OutOfFold([a, b], [[0], [1], [2]])
    with pytest.raises(ValueError, match=r"different classes_ \(7 and 6 classes\)"):
        OutOfFold([a, fitted(7)], folds)
    with pytest.raises(RuntimeError, match="initialized"):
        OutOfFold([a, NeuralNetClassifier(module="model.Transformer")], folds)
    with pytest.raises(ValueError, match="member 1 is on cuda:1"):
        OutOfFold([a, fitted(6, "cuda:1")], folds)
    with pytest.raises(ValueError, match="dataset must be the TokenDataset of the 5 rows"):
        OutOfFold([a, b], folds, dataset="rows")
    assert check_partition("x", [[1, 0], [2]])[1] == 3
    # another data set is refused before any forward pass
    from slnlp.data import TokenDataset
    ds = TokenDataset(np.zeros((5, 3)), np.full(5, 3), np.arange(5))
    other = TokenDataset(np.ones((5, 3)), np.full(5, 3), np.arange(5))
    bound = OutOfFold([a, b], folds, dataset=ds)
    for wrong in (other, ds[np.arange(4)]):
        with pytest.raises(ValueError, match="out-of-fold log-probs exist only for the 5 rows"):
            bound._forward_logp(wrong, lambda logp, yd: None)
    with pytest.raises(TypeError, match="cross_fit: dataset must be"):
        cross_fit(a, {"X": 0})
    with pytest.raises(ValueError, match="cross_fit: cv=1"):
        cross_fit(a, ds, cv=1)


def test_cli_key_is_validated():
    from slnlp import cli
    assert cli.label_audit_options(None) is None and "label_audit" in cli.DICT_ARGS
    assert cli.label_audit_options({}) == {"cv": 5, "rank_by": "normalized_margin", "pairs": 20, "top": 200}
    assert cli.label_audit_options({"cv": 2, "rank_by": "self_confidence", "pairs": 1, "top": 0}) == \
        {"cv": 2, "rank_by": "self_confidence", "pairs": 1, "top": 0}
    for bad, text in (([], "expected a dict"), ({"folds": 3}, "unknown keys"), ({"cv": 1}, "cv=1"), ({"cv": 33}, "cv=33"), ({"cv": 2.0}, "cv=2.0"),
                      ({"cv": True}, "cv=True"), ({"rank_by": "margin"}, "rank_by='margin'"), ({"pairs": 0}, "pairs=0"), ({"pairs": 65}, "pairs=65"),
                      ({"top": -1}, "top=-1"), ({"top": "all"}, "top='all'")):
        with pytest.raises(ValueError, match=text):
            cli.label_audit_options(bad)


def test_label_issues_checks_come_before_the_forward_pass():
    from slnlp.net import NeuralNetClassifier
    net = NeuralNetClassifier(module="model.Transformer")
    with pytest.raises(RuntimeError, match="not initialized"):
        net.label_issues(None)
    net.initialized_, net.classes_ = True, np.arange(6)
    with pytest.raises(ValueError, match="label_issues: rank_by='margin'"):
        net.label_issues(None, rank_by="margin")
    with pytest.raises(ValueError, match="label_issues: pairs=0"):
        net.label_issues(None, pairs=0)
    net.classes_ = np.arange(4097)
    with pytest.raises(ValueError, match="label_issues: 4097 classes"):
        net.label_issues(None)


def test_scale_restatement_is_a_log_softmax():
    import conformal_ref as cr
    z, _ = cr.make_logp(9, 7, 5)
    for beta in (0.5, 1.0, 2.0):
        out = lr.scale_ref(z, beta).astype(np.float64)
        assert np.abs(np.exp(out).sum(axis=1) - 1.0).max() < 1e-6
        assert np.abs((out - out[:, :1]) - beta * (z - z[:, :1]).astype(np.float64)).max() < 1e-5
