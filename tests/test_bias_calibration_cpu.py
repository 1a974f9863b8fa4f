"""CPU: the host side of the ``bias_temperature`` calibration -- the numpy restatement the GPU tests lean on
(tests/bias_calibration_ref.py) against scipy's L-BFGS-B with the analytic gradient, the monotone objective, the condition that
keeps the GPU comparison meaningful (every GPU input converges inside the cap), option parsing and the checkpoint's dict."""
import json
import os
import re

import numpy as np
import pytest

from bias_calibration_ref import (EVALS, _rows, decisions_are_clear, evaluate, fit_bias_temperature_ref, kernel_cases, make_shifted_logp, newton_direction,
                                  shift_logp_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIAS = {"method": "bias_temperature", "bias_sd": 2.0}
TOL = 1e-10


# ------------------------------------------------------------------------------------------------- the restatement ----
def _against_scipy(N, V, seed, bias_sd):
    """``(the restatement's result, F and g at it, scipy's F)``; F agrees to 1e-10 and is not above scipy's."""
    from scipy.optimize import minimize
    logp, y = make_shifted_logp(N, V, seed)
    z, yk, _ = _rows(logp, y)
    got = fit_bias_temperature_ref(logp, y, bias_sd, TOL)
    theta = np.concatenate([[got["beta"]], got["bias"]])
    F, g, _ = evaluate(z, yk, theta, bias_sd, hessian=False)
    fun = lambda t: evaluate(z, yk, t, bias_sd, hessian=False)[:2]
    res = minimize(fun, np.concatenate([[1.0], np.zeros(V)]), jac=True, method="L-BFGS-B", bounds=[(2.0 ** -6, 2.0 ** 6)] + [(None, None)] * V,
                   options={"maxiter": 20000, "maxfun": 200000, "ftol": 1e-16, "gtol": 1e-9, "maxcor": 50})
    print(f"[{N} x {V} sd {bias_sd}] F = {F!r} (scipy {res.fun!r} after {res.nit} iterations), |g|_inf = {np.abs(g).max():.3e}, "
          f"{got['reason']} after {got['iterations']} evaluations, {got['halvings']} halvings, beta {got['beta']:.6f}")
    assert abs(F - res.fun) <= 1e-10, (F, res.fun)
    assert F <= res.fun + 1e-15                              # the Newton iterate is the better minimiser of a convex F
    assert abs(got["nll_after"] + got["penalty"] - F) <= 1e-14 * max(1.0, abs(F))
    return got, g


@pytest.mark.parametrize("N,V,seed", [(64, 5, 11), (257, 33, 12), (300, 202, 13)])
@pytest.mark.parametrize("bias_sd", [2.0, 8.0])
def test_ref_against_scipy(N, V, seed, bias_sd):
    got, g = _against_scipy(N, V, seed, bias_sd)
    assert got["reason"] == "gradient" and got["iterations"] <= EVALS
    assert np.abs(g).max() <= TOL


@pytest.mark.parametrize("N,V,seed", [(64, 5, 11), (257, 33, 12), (300, 202, 13)])
def test_under_a_tight_prior_the_search_may_end_at_the_round_off_floor_of_f(N, V, seed):
    """The Armijo test compares two evaluations of F, each good to a few ulp: a step whose predicted decrease g^T d is of the order
    of 2^-52 F cannot be verified and is halved until the cap -- here at bias_sd = 0.5 on 300 x 202, where the search ends with
    reason "cap" at |g|_inf = 2.8e-9.  Since g^T H^-1 g >= |g|^2 / lambda_max(H) and lambda_max is O(1) for log-probs of this
    scale, a stall needs |g| below about sqrt(1e-15 F), i.e. 1e-7: the minimiser is found all the same (F agrees with scipy's to
    1e-10), only the 1e-10 gradient test is out of reach.  The estimator warns for "cap" and keeps the result."""
    got, g = _against_scipy(N, V, seed, 0.5)
    assert got["reason"] in ("gradient", "cap") and got["iterations"] <= EVALS
    assert np.abs(g).max() <= (TOL if got["reason"] == "gradient" else 1e-7)


@pytest.mark.parametrize("bias_sd", [0.5, 2.0, 8.0])
def test_f_never_increases_over_accepted_steps(bias_sd):
    for N, V, seed in [(3, 2, 1), (64, 5, 11), (257, 33, 12), (300, 202, 13)]:
        got = fit_bias_temperature_ref(*make_shifted_logp(N, V, seed), bias_sd, TOL)
        trace = got["trace"]
        assert len(trace) >= 2 and all(b <= a for a, b in zip(trace, trace[1:])), (N, V, trace)
        assert got["nll_after"] <= got["nll_before"]


def test_every_gpu_input_ends_with_reason_gradient_inside_the_cap():
    """... and by decisions none of which was close (``decisions_are_clear``): the device sums in another order, which moves F and
    g by a few ulp, so a run whose every comparison is decided by hundreds of ulp takes the same steps there."""
    rejected = box = 0
    for name, logp, y, ld, bias_sd in kernel_cases():
        got = fit_bias_temperature_ref(logp, y, bias_sd, TOL)
        turned_down = sum(1 for kind, a, b in got["decisions"] if kind == "armijo" and not a <= b)
        print(f"[{name}] {got['reason']} after {got['iterations']} evaluations, {turned_down} rejected, {got['halvings']} halvings, "
              f"beta {got['beta']:.6f}, nll {got['nll_before']:.6f} -> {got['nll_after']:.6f}")
        if logp.shape[1] == 1:
            assert (got["reason"], got["iterations"], got["beta"]) == ("flat", 0, 1.0) and not got["bias"].any()
        else:
            assert got["reason"] == "gradient" and 2 <= got["iterations"] < EVALS and decisions_are_clear(got), name
        rejected += turned_down
        box += got["halvings"] - turned_down
    assert rejected >= 2 and box >= 2, "the cases no longer take the reject path or the box halvings"
    wide = [c for c in kernel_cases() if c[0].startswith("N300_V202")][0]
    assert not (wide[2] == 17).any() and ((wide[2] < 0) | (wide[2] >= 202)).sum() == 3


def test_analytic_gradient_and_hessian_against_differences():
    logp, y = make_shifted_logp(40, 7, 5)
    z, yk, _ = _rows(logp, y)
    rng = np.random.default_rng(0)
    theta = np.concatenate([[1.3], 0.3 * rng.normal(size=7)])
    F, g, H = evaluate(z, yk, theta, 2.0)
    h = 1e-6
    for i in range(8):
        e = np.zeros(8)
        e[i] = h
        Fp, gp, _ = evaluate(z, yk, theta + e, 2.0, hessian=False)
        Fm, gm, _ = evaluate(z, yk, theta - e, 2.0, hessian=False)
        assert abs((Fp - Fm) / (2 * h) - g[i]) <= 1e-8
        assert np.abs((gp - gm) / (2 * h) - H[:, i]).max() <= 1e-8
    assert np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() > 0.0
    assert np.abs(newton_direction(H, g) + np.linalg.solve(H, g)).max() <= 1e-12
    assert newton_direction(-H, g) is None


def test_labels_out_of_range_are_counted_and_excluded():
    logp, y = make_shifted_logp(50, 6, 9)
    keep = np.ones(50, dtype=bool)
    keep[[4, 17]] = False
    bad = y.copy()
    bad[4], bad[17] = -1, 6
    a, b = fit_bias_temperature_ref(logp, bad), fit_bias_temperature_ref(logp[keep], y[keep])
    assert (a["rows"], a["bad_labels"], b["bad_labels"]) == (48, 2, 0)
    assert a["beta"] == b["beta"] and np.array_equal(a["bias"], b["bias"])
    none = fit_bias_temperature_ref(logp, np.full(50, -1))
    assert (none["reason"], none["rows"], none["beta"], none["nll_before"], none["nll_after"]) == ("flat", 0, 1.0, 0.0, 0.0)


def test_the_bias_removes_a_prior_mismatch_a_temperature_cannot():
    from calibration_ref import fit_temperature_ref
    logp, y = make_shifted_logp(800, 40, 21)
    fresh, yf = make_shifted_logp(4000, 40, 22)
    t, b = fit_temperature_ref(logp, y), fit_bias_temperature_ref(logp, y)
    nll = lambda lp: float(-lp[np.arange(len(yf)), yf].mean())
    plain, temp, both = nll(fresh.astype(np.float64)), nll(shift_logp_ref(fresh, t["beta"], 0.0)), nll(shift_logp_ref(fresh, b["beta"], b["bias"]))
    print(f"fresh rows: log-loss {plain:.4f}, temperature {temp:.4f}, bias_temperature {both:.4f}")
    assert both < temp < plain


# ------------------------------------------------------------------------------------------------------ the option ----
def test_calibration_options():
    from slnlp.net import calibration_options
    assert calibration_options(BIAS) == BIAS
    assert calibration_options({"method": "bias_temperature"}) == BIAS                   # the default bias_sd
    assert calibration_options({"method": "bias_temperature", "bias_sd": 1}) == {"method": "bias_temperature", "bias_sd": 1.0}
    assert calibration_options({"method": "bias_temperature", "bias_sd": np.float32(0.5)})["bias_sd"] == 0.5
    assert calibration_options({"method": "temperature"}) == {"method": "temperature"} and calibration_options(None) is None


@pytest.mark.parametrize("bad", [{"method": "bias_temperature", "bias_sd": 0.0}, {"method": "bias_temperature", "bias_sd": -1.0},
                                 {"method": "bias_temperature", "bias_sd": float("inf")}, {"method": "bias_temperature", "bias_sd": float("nan")},
                                 {"method": "bias_temperature", "bias_sd": "2"}, {"method": "bias_temperature", "bias_sd": True},
                                 {"method": "bias_temperature", "bias_sd": None}, {"method": "bias_temperature", "tol": 1e-8},
                                 {"method": "temperature", "bias_sd": 2.0}, {"bias_sd": 2.0}, {"method": "bias", "bias_sd": 2.0}])
def test_bad_options_raise_value_error(bad):
    from slnlp.net import NeuralNetClassifier, calibration_options
    with pytest.raises(ValueError, match="calibration"):
        calibration_options(bad)
    with pytest.raises(ValueError, match="calibration"):
        NeuralNetClassifier(module="model.Transformer", calibration=bad).initialize()


def test_what_was_refused_before_is_refused_in_the_same_words():
    from slnlp.net import calibration_options
    for bad, text in [({"method": "temperature", "bias_sd": 2.0}, r"unknown keys \['bias_sd'\] \(known: \('method',\)\)"),
                      ({"bias_sd": 2.0}, r"unknown keys \['bias_sd'\] \(known: \('method',\)\)"),
                      ({"method": "platt"}, "method='platt', expected 'temperature'"),
                      ("bias_temperature", "expected a dict with keys among")]:
        with pytest.raises(ValueError, match=text):
            calibration_options(bad)


def test_sklearn_surface_grid_axis_and_cli():
    from slnlp import cli, grid
    from slnlp.data import synthetic_dataset
    from slnlp.net import NeuralNetClassifier
    net = NeuralNetClassifier(module="model.Transformer", calibration=BIAS)
    assert net.get_params()["calibration"] == BIAS and NeuralNetClassifier(**net.get_params()).get_params()["calibration"] == BIAS
    with pytest.raises(ValueError, match="train_split"):
        NeuralNetClassifier(module="model.Transformer", calibration=BIAS, train_split=None).initialize()
    ds = synthetic_dataset(48, seq_len=8, src_vocab=40, n_labels=4, seed=3, min_len=3)
    axis = [None, {"method": "temperature"}, BIAS, {"method": "bias_temperature", "bias_sd": 0.5}]
    cands, folds, tasks, order = grid.build_tasks({"lr": [0.1], "calibration": axis}, ds.y, 2)
    units = grid.build_units(cands, folds, tasks, order, lockstep=8)
    assert len(tasks) == 8 and len(units) == 1                                           # a LOCKSTEP_NEUTRAL key: one unit

    class _Vocab:
        stoi = {"<pad>": 1}

    class _Data:
        vocab_X = vocab_y = _Vocab()
    assert cli.build_net_params({"model": "model.Transformer", "calibration": BIAS}, _Data(), "cuda")["calibration"] == BIAS
    assert cli.build_param_grid({"calibration": axis}) == {"calibration": axis}


# -------------------------------------------------------------------------------------------------- the checkpoint ----
def test_checkpoint_round_trip_of_the_dict(tmp_path):
    from slnlp.net import calibration_from_json, calibration_to_json
    got = fit_bias_temperature_ref(*make_shifted_logp(64, 5, 1))
    info = {k: got[k] for k in ("temperature", "beta", "nll_before", "nll_after", "reason", "iterations", "rows", "bad_labels", "method",
                                "bias_sd", "bias", "penalty")}
    with open(tmp_path / "calibration.json", "w") as f:
        json.dump(calibration_to_json(info), f, indent=1)
    with open(tmp_path / "calibration.json") as f:
        back = calibration_from_json(json.load(f))
    assert list(back) == list(info)
    assert back["bias"].dtype == np.float64 and back["bias"].tobytes() == info["bias"].tobytes()        # bit for bit
    assert all(back[k] == info[k] for k in info if k != "bias")
    temperature = {"temperature": 1.25, "beta": 0.8, "reason": "gradient"}                              # a temperature fit's dict: untouched
    assert calibration_to_json(temperature) == temperature and calibration_from_json(temperature) == temperature


# ----------------------------------------------------------------------------------------------------------- C ABI ----
def test_entry_points_are_declared_and_bound():
    from slnlp import _lib
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(slnlp_[a-z0-9_]+)\s*\(", src))
    for name in ("slnlp_fit_bias_temperature", "slnlp_fit_bias_temperature_scratch_bytes"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["slnlp_fit_bias_temperature"][1]) == 12
    codes = dict(re.findall(r"#define SLNLP_CAL_([A-Z]+) (\d+)", src))
    assert {int(v): k.lower() for k, v in codes.items() if k != "STATE"} == _lib.BIAS_CALIBRATION_REASONS
    assert int(re.search(r"#define SLNLP_BIAS_CAL_MAX_V (\d+)", src).group(1)) == _lib.BIAS_CAL_MAX_V == 512
