"""CPU: the host side of ``calibration`` -- the numpy restatement the GPU tests lean on (tests/calibration_ref.py) against scipy's
bounded scalar minimiser, its edge rules, the option's validation, the grid grouping and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

from calibration_ref import fit_temperature_ref, scale_logp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPERATURE = {"method": "temperature"}


def make_logp(N, V, scale, boosted, seed):
    """float32 log-softmax of ``scale * randn`` logits [N, V] whose true class got ``+ 4 scale`` in a fraction ``boosted`` of the
    rows, and the labels."""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, V, size=N)
    logits = scale * rs.randn(N, V)
    rows = np.flatnonzero(rs.rand(N) < boosted)
    logits[rows, y[rows]] += 4.0 * scale
    logits -= logits.max(axis=1, keepdims=True)
    logp = logits - np.log(np.exp(logits).sum(axis=1, keepdims=True))
    return logp.astype(np.float32), y.astype(np.int64)


CASES = [(257, 70, 8.0, 0.6), (257, 70, 0.3, 0.9), (5, 3, 2.0, 0.6)]
INPUTS = [(c, seed) for c in CASES for seed in (1, 2, 3)]


def _nll(logp, y, beta):
    return float(-scale_logp_ref(logp, beta)[np.arange(len(y)), y].mean())


@pytest.mark.parametrize("case,seed", INPUTS)
def test_ref_against_scipy_bounded(case, seed):
    from scipy.optimize import minimize_scalar
    logp, y = make_logp(*case, seed)
    got = fit_temperature_ref(logp, y)
    res = minimize_scalar(lambda u: _nll(logp, y, np.exp(u)), bounds=(-6 * np.log(2.0), 6 * np.log(2.0)), method="bounded",
                          options={"xatol": 1e-12})
    T = float(np.exp(-res.x))
    print(f"[{case} seed {seed}] T = {got['temperature']:.12g} (scipy {T:.12g}), {got['reason']} after {got['iterations']} iterations, "
          f"nll {got['nll_before']:.6f} -> {got['nll_after']:.6f}")
    # the cap cannot hide a failure: the search ended on its own, early
    assert got["reason"] in ("gradient", "step") and got["iterations"] <= 16
    assert abs(got["temperature"] / T - 1.0) <= 1e-6
    assert got["nll_after"] <= got["nll_before"]
    assert got["rows"] == case[0] and got["bad_labels"] == 0
    assert got["beta"] == 1.0 / got["temperature"] or abs(got["beta"] * got["temperature"] - 1.0) <= 2 ** -52
    assert abs(got["nll_after"] - _nll(logp, y, got["beta"])) <= 1e-12 * max(1.0, got["nll_after"])


def test_the_two_big_cases_sit_where_the_issue_says():
    """An overconfident model wants T well above 1, an underconfident one well below."""
    assert fit_temperature_ref(*make_logp(257, 70, 8.0, 0.6, 1))["temperature"] > 3.0
    assert fit_temperature_ref(*make_logp(257, 70, 0.3, 0.9, 1))["temperature"] < 0.3


def test_edge_rules():
    flat = fit_temperature_ref(np.full((9, 4), np.log(0.25), dtype=np.float32), np.arange(9) % 4)
    assert (flat["temperature"], flat["reason"], flat["iterations"]) == (1.0, "flat", 0)
    assert flat["nll_after"] <= flat["nll_before"]
    two = np.log(np.array([[0.9, 0.1]], dtype=np.float32))
    wrong = fit_temperature_ref(two, np.array([1]))                 # the wrong class is favoured: as flat as allowed
    assert (wrong["temperature"], wrong["beta"], wrong["reason"]) == (64.0, 2.0 ** -6, "bound")
    right = fit_temperature_ref(two, np.array([0]))                 # the right one: as sharp as allowed
    assert (right["temperature"], right["beta"], right["reason"]) == (1.0 / 64.0, 64.0, "bound")
    for r in (wrong, right):
        assert r["nll_after"] <= r["nll_before"] and r["iterations"] == 0


def test_labels_out_of_range_are_counted_and_excluded():
    logp, y = make_logp(33, 7, 2.0, 0.6, 4)
    bad = y.copy()
    bad[3], bad[20] = -1, 7
    got = fit_temperature_ref(logp, bad)
    keep = np.ones(33, dtype=bool)
    keep[[3, 20]] = False
    want = fit_temperature_ref(logp[keep], y[keep])
    assert got["bad_labels"] == 2 and got["rows"] == 31
    assert {k: v for k, v in got.items() if k != "bad_labels"} == {k: v for k, v in want.items() if k != "bad_labels"}
    none = fit_temperature_ref(logp[:2], np.array([-5, 99]))
    assert (none["rows"], none["bad_labels"], none["temperature"], none["reason"]) == (0, 2, 1.0, "flat")


@pytest.mark.parametrize("beta", [2.0 ** -6, 0.37, 1.0, 5.5, 64.0])
def test_scale_logp_ref_normalises_and_keeps_the_argmax(beta):
    logp, _ = make_logp(257, 70, 8.0, 0.6, 2)
    out = scale_logp_ref(logp, beta)
    assert out.dtype == np.float64 and out.shape == logp.shape
    assert np.abs(np.log(np.exp(out).sum(axis=1))).max() <= 1e-12
    assert np.array_equal(out.argmax(axis=1), logp.argmax(axis=1))


# ------------------------------------------------------------------------------------------------------ the option ----
def test_calibration_options():
    from slnlp.net import calibration_options
    assert calibration_options(None) is None and calibration_options(False) is None
    assert calibration_options(TEMPERATURE) == TEMPERATURE
    assert calibration_options({}) == TEMPERATURE


@pytest.mark.parametrize("bad", [{"method": "temperature", "bins": 10}, {"method": "platt"}, {"method": None}, "temperature", True, 1.5,
                                 [TEMPERATURE]])
def test_bad_options_raise_value_error(bad):
    from slnlp.net import NeuralNetClassifier, calibration_options
    with pytest.raises(ValueError, match="calibration"):
        calibration_options(bad)
    # ... and from initialize(), before anything else of the fit is set up (so also on a machine without a GPU)
    with pytest.raises(ValueError, match="calibration"):
        NeuralNetClassifier(module="model.Transformer", calibration=bad).initialize()


def test_sklearn_surface_and_the_valid_split_requirement():
    from slnlp.net import NeuralNetClassifier
    net = NeuralNetClassifier(module="model.Transformer")
    assert "calibration" in NeuralNetClassifier._OWN and net.get_params()["calibration"] is None      # default off
    net.set_params(calibration=TEMPERATURE)
    assert net.get_params()["calibration"] == TEMPERATURE and net.calibration == TEMPERATURE
    assert NeuralNetClassifier(**net.get_params()).get_params()["calibration"] == TEMPERATURE
    for split in (None, 0, False):                       # nothing held out: nothing to fit the temperature on
        with pytest.raises(ValueError, match="train_split"):
            NeuralNetClassifier(module="model.Transformer", calibration=TEMPERATURE, train_split=split).initialize()


def test_calibration_does_not_split_lockstep_units():
    from slnlp import grid
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(48, seq_len=8, src_vocab=40, n_labels=4, seed=3, min_len=3)
    assert "calibration" in grid.SHAPE_KEYS_EXCLUDED
    cands, folds, tasks, order = grid.build_tasks({"lr": [0.1], "calibration": [None, TEMPERATURE]}, ds.y, 2)
    units = grid.build_units(cands, folds, tasks, order, lockstep=8)
    assert len(tasks) == 4 and len(units) == 1 and sorted(units[0]) == list(range(4))


def test_cli_passes_the_key_through():
    from slnlp import cli

    class _Vocab:
        stoi = {"<pad>": 1}

    class _Data:
        vocab_X = vocab_y = _Vocab()
    base = {"model": "model.Transformer"}
    assert "calibration" not in cli.build_net_params(base, _Data(), "cuda")
    assert cli.build_net_params(dict(base, calibration=TEMPERATURE), _Data(), "cuda")["calibration"] == TEMPERATURE
    assert cli.build_param_grid({"calibration": [None, TEMPERATURE]}) == {"calibration": [None, TEMPERATURE]}


# ----------------------------------------------------------------------------------------------------------- C ABI ----
def test_both_entry_points_are_declared_and_bound():
    from slnlp import _lib
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                  # the way tests/test_abi.py reads the header
    declared = set(re.findall(r"\b(slnlp_[a-z0-9_]+)\s*\(", src))
    for name in ("slnlp_fit_temperature", "slnlp_fit_temperature_scratch_bytes", "slnlp_scale_logp"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["slnlp_fit_temperature"][1]) == 9 and len(_lib.SIGNATURES["slnlp_scale_logp"][1]) == 8
    codes = dict(re.findall(r"#define SLNLP_CAL_(FLAT|BOUND|GRADIENT|STEP|CAP) (\d+)", src))
    assert {int(v): k.lower() for k, v in codes.items()} == _lib.CALIBRATION_REASONS
