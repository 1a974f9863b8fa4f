"""GPU: bias-corrected temperature calibration fitted on the device -- ``slnlp_fit_bias_temperature`` through the C ABI against the
numpy restatement (tests/bias_calibration_ref.py, itself held to scipy on the CPU), and the estimator's ``calibration`` option with
``method="bias_temperature"`` on the solo path, in a lockstep group and through every wrapper that judges log-probs.

The bounds are derived, not chosen (``_held_to_the_restatement`` says why each holds):
  * the restatement's gradient AT the device's result: |g|_inf <= tol + 64 N 2^-53 (row scale) -- the project's summation bound;
  * ``nll_after`` against the restatement's log-loss AT the device's result, ``nll_before`` against the restatement's: 1e-12
    relative, tests/test_calibration_gpu.py's bound and reasoning;
  * |theta_dev - theta_ref|_inf <= 2 (|H^-1 g(theta_dev)|_inf + |H^-1 g(theta_ref)|_inf) + 2^-40 max(1, |theta|_inf): both points
    lie within about one Newton step of the minimiser of a convex F, H and g from the restatement.
The kernel inputs are tests/bias_calibration_ref.py's ``kernel_cases``: the CPU suite checks that the restatement ends each with
reason "gradient" by decisions none of which was close, so the device must take the same steps: same reason, same count."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from bias_calibration_ref import _rows, evaluate, fit_bias_temperature_ref, kernel_cases, make_shifted_logp, nll, shift_logp_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPERATURE = {"method": "temperature"}
BIAS = {"method": "bias_temperature", "bias_sd": 2.0}
TOL = 1e-10


def _device(logp, y, ld=None):
    """``logp`` on the device, its rows ``ld`` floats apart (the padding is NaN: never to be read), and the labels."""
    N, V = logp.shape
    buf = torch.full((N, ld or V), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(logp).cuda()
    return buf[:, :V], torch.from_numpy(np.asarray(y, dtype=np.int64)).cuda()


def _held_to_the_restatement(name, logp, y, bias_sd, got, want, tol=TOL):
    """The three bounds of the module docstring for the device's result ``got`` (``ops.bias_temperature_download``'s dict) against the
    restatement's ``want`` on the float32 log-probs ``logp``; returns the measured figures."""
    z, yk, _ = _rows(logp, y)
    N, M = logp.shape[0], len(yk)
    dev, ref = np.concatenate([[got["beta"]], got["bias"]]), np.concatenate([[want["beta"]], want["bias"]])
    _, g_dev, H_dev = evaluate(z, yk, dev, bias_sd)
    _, g_ref, H_ref = evaluate(z, yk, ref, bias_sd)
    # every entry of g is a mean of M terms of size at most (row scale): p <= 1 for the biases, |m_i - z_iy| <= 2 max |z| for beta,
    # plus lambda |b|; the device adds them in another order and its exp / log differ from numpy's by a few ulp
    scale = 1.0 + 2.0 * float(np.abs(z).max()) + float(np.abs(dev[1:]).max()) / (bias_sd * bias_sd * M)
    g_bound = tol + 64.0 * N * 2.0 ** -53 * scale
    g_inf = float(np.abs(g_dev).max())
    # the same fp64 sums of M terms on both sides: rounding of order sqrt(M) 2^-53, far below 1e-12
    after = nll(z, yk, dev)
    nll_err = max(abs(got["nll_after"] - after) / abs(after), abs(got["nll_before"] - want["nll_before"]) / abs(want["nll_before"]))
    # F is convex and both points passed the gradient test: each lies within its own Newton step |H^-1 g| of the minimiser up to
    # the step's second-order term, which the factor 2 covers; 2^-40 relative covers the rounding of theta itself
    step_dev, step_ref = float(np.abs(np.linalg.solve(H_dev, g_dev)).max()), float(np.abs(np.linalg.solve(H_ref, g_ref)).max())
    theta_bound = 2.0 * (step_dev + step_ref) + 2.0 ** -40 * max(1.0, float(np.abs(ref).max()))
    theta_err = float(np.abs(dev - ref).max())
    rec = {"reason": got["reason"], "evaluations": got["iterations"], "beta": got["beta"], "g_inf_at_device_theta": g_inf, "g_bound": g_bound,
           "nll_relative_error": nll_err, "theta_deviation": theta_err, "theta_bound": theta_bound, "newton_step_device": step_dev,
           "newton_step_restatement": step_ref}
    print(f"[{name}] {rec}")
    assert g_inf <= g_bound, (name, rec)
    assert nll_err <= 1e-12, (name, rec)
    assert theta_err <= theta_bound, (name, rec)
    assert abs(got["penalty"] - 0.5 / (bias_sd * bias_sd * M) * float((got["bias"] ** 2).sum())) <= 1e-15 * max(1.0, got["penalty"])
    return rec


@pytest.fixture(scope="module")
def refs():
    """The restatement on every kernel case, once."""
    return {name: fit_bias_temperature_ref(logp, y, sd, TOL) for name, logp, y, ld, sd in kernel_cases()}


# ------------------------------------------------------------------------------------------------- kernels, C ABI ----
def test_fit_against_the_restatement(refs):
    from slnlp import ops
    worst = {"g_inf_over_bound": 0.0, "nll_relative_error": 0.0, "theta_deviation_over_bound": 0.0, "cases": {}}
    for name, logp, y, ld, sd in kernel_cases():
        want = refs[name]
        state, bias = ops.fit_bias_temperature(*_device(logp, y, ld), bias_sd=sd, tol=TOL)
        got = ops.bias_temperature_download(state, bias, sd)
        print(f"[{name}] device {got['reason']} after {got['iterations']}, beta {got['beta']!r}; ref {want['reason']} after "
              f"{want['iterations']}, beta {want['beta']!r}")
        assert (got["reason"], got["rows"], got["bad_labels"]) == (want["reason"], want["rows"], want["bad_labels"]), name
        assert got["iterations"] == want["iterations"], (name, got["iterations"], want["iterations"])
        assert got["temperature"] == 1.0 / got["beta"] and (got["method"], got["bias_sd"]) == ("bias_temperature", sd), name
        assert got["bias"].dtype == np.float64 and got["bias"].shape == (logp.shape[1],), name
        if logp.shape[1] == 1:
            assert (got["beta"], got["nll_before"], got["nll_after"], got["penalty"]) == (1.0, 0.0, 0.0, 0.0) and not got["bias"].any()
            worst["cases"][name] = {"reason": got["reason"], "evaluations": 0}
            continue
        rec = _held_to_the_restatement(name, logp, y, sd, got, want)
        assert got["nll_after"] <= got["nll_before"], name
        worst["cases"][name] = rec
        worst["g_inf_over_bound"] = max(worst["g_inf_over_bound"], rec["g_inf_at_device_theta"] / rec["g_bound"])
        worst["nll_relative_error"] = max(worst["nll_relative_error"], rec["nll_relative_error"])
        worst["theta_deviation_over_bound"] = max(worst["theta_deviation_over_bound"], rec["theta_deviation"] / rec["theta_bound"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bias_calibration_parity.json"), "w") as f:
        json.dump({"test": "tests/test_bias_calibration_gpu.py::test_fit_against_the_restatement", "device": torch.cuda.get_device_name(0),
                   "tol": TOL, "nll_bound": 1e-12, **worst}, f, indent=1)
        f.write("\n")


def test_an_absent_class_gets_a_negative_bias_and_excluded_rows_change_nothing():
    from slnlp import ops
    (name, logp, y, ld, sd), = [c for c in kernel_cases() if c[0].startswith("N300_V202")]
    state, bias = ops.fit_bias_temperature(*_device(logp, y, ld), bias_sd=sd)
    got = ops.bias_temperature_download(state, bias, sd)
    assert got["bias"][17] < 0.0 and got["bad_labels"] == 3 and got["rows"] == 297
    keep = (y >= 0) & (y < 202)
    state2, bias2 = ops.fit_bias_temperature(*_device(logp[keep], y[keep]), bias_sd=sd)
    other = ops.bias_temperature_download(state2, bias2, sd)
    # the same objective: an excluded row adds zeros to every sum.  Which thread adds which row differs, so the two results are
    # held to the same restatement run by the derived bounds, not to each other bit for bit
    want = fit_bias_temperature_ref(logp[keep], y[keep], sd)
    assert (other["rows"], other["bad_labels"], other["reason"], other["iterations"]) == (297, 0, got["reason"], got["iterations"])
    _held_to_the_restatement(name + " without the excluded rows", logp[keep], y[keep], sd, other, want)
    _held_to_the_restatement(name + " against the run without them", logp, y, sd, got, want)


def test_the_result_is_a_pure_function_of_the_arguments():
    from slnlp import _lib, ops
    (name, logp, y, ld, sd), = [c for c in kernel_cases() if c[0].startswith("N257_V17")]
    z, yd = _device(logp, y, ld)
    doubles = _lib.load().slnlp_fit_bias_temperature_scratch_bytes(257, 17) // 8
    state, bias, scratch = (torch.zeros(n, dtype=torch.float64, device="cuda") for n in (16, 17, doubles))
    bits = lambda pair: pair[0].cpu().numpy().tobytes() + pair[1].cpu().numpy().tobytes()
    first = bits(ops.fit_bias_temperature(z, yd, bias_sd=sd, state=state, bias=bias, scratch=scratch))
    assert bits(ops.fit_bias_temperature(z, yd, bias_sd=sd, state=state, bias=bias, scratch=scratch)) == first     # over its own leftovers
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    assert bits(ops.fit_bias_temperature(z, yd, bias_sd=sd, state=nan(16), bias=nan(17), scratch=nan(doubles + 64))) == first
    assert bits(ops.fit_bias_temperature(z, yd, bias_sd=sd)) == first
    assert np.isfinite(np.frombuffer(first, dtype=np.float64)[:4]).all()


def test_a_loose_tolerance_stops_at_the_start_and_the_state_serves_the_consumers():
    from slnlp import ops
    logp, y = make_shifted_logp(33, 7, 3)
    z, yd = _device(logp, y)
    state, bias = ops.fit_bias_temperature(z, yd, tol=1e6)
    got = ops.bias_temperature_download(state, bias, 2.0)
    assert (got["reason"], got["iterations"], got["beta"]) == ("gradient", 1, 1.0) and not got["bias"].any()
    assert got["nll_before"] == got["nll_after"]
    state, bias = ops.fit_bias_temperature(z, yd)
    got = ops.bias_temperature_download(state, bias, 2.0)
    out = ops.shift_logp(z, bias, state=state).cpu().numpy()
    want = shift_logp_ref(logp, got["beta"], got["bias"])
    w32 = want.astype(np.float32)
    assert (np.abs(out.astype(np.float64) - want) / np.spacing(np.abs(w32)).astype(np.float64)).max() <= 1.0      # one float32 ulp
    st2, b2 = ops.bias_temperature_state(got["beta"], got["bias"], "cuda")
    assert torch.equal(ops.shift_logp(z, b2, state=st2), torch.from_numpy(out).cuda())                           # read back from a checkpoint
    assert -float(want[np.arange(33), y].mean()) == pytest.approx(got["nll_after"], rel=1e-12)


def test_bad_arguments_return_codes_and_messages():
    from slnlp import _lib, ops
    lib = _lib.load()
    z, y = _device(*make_shifted_logp(5, 3, 1))
    need = lib.slnlp_fit_bias_temperature_scratch_bytes(5, 3)
    assert need == 8 * (5 * 16 + 3 * 16 + 4 * 32 + 4 * 32 + 4 * 5)
    state, bias, scratch = (torch.zeros(n, dtype=torch.float64, device="cuda") for n in (16, 3, need // 8))
    p, st = _lib.ptr, _lib.stream_ptr()
    for N, V, text in [(0, 3, "N=0"), (5, 0, "V=0"), (5, 513, "V=513"), (2 ** 31, 3, "N=2147483648")]:
        assert lib.slnlp_fit_bias_temperature_scratch_bytes(N, V) == -1 and text in lib.slnlp_last_error().decode()
    assert lib.slnlp_fit_bias_temperature_scratch_bytes(5, 512) > 0
    fit = lambda *a: (lib.slnlp_fit_bias_temperature(*a, st), lib.slnlp_last_error().decode())
    ok = (p(z), 3, p(y), 5, 3, 2.0, 1e-10, p(state), p(bias), p(scratch), need)
    for i, value, text in [(0, None, "null pointer"), (2, None, "null pointer"), (7, None, "null pointer"), (8, None, "null pointer"),
                           (9, None, "null pointer"), (1, 2, "ld=2 is less than V=3"), (3, 0, "N=0"), (4, 0, "V=0"), (4, 513, "V=513 outside 1..512"),
                           (5, 0.0, "bias_sd=0"), (5, -1.0, "bias_sd=-1"), (5, float("inf"), "bias_sd=inf"), (5, float("nan"), "bias_sd=nan"),
                           (6, -1e-3, "tol=-0.001"), (6, float("inf"), "tol=inf"), (6, float("nan"), "tol=nan"),
                           (10, need - 1, "too small"), (9, p(scratch) + 8, "32-byte aligned"), (8, p(bias) + 4, "misaligned"),
                           (7, p(scratch), "overlap"), (8, p(state), "overlap"), (8, p(y), "overlaps input y"), (9, p(z), "overlap")]:
        args = list(ok)
        args[i] = value
        rc, msg = fit(*args)
        assert rc == 1 and text in msg, (i, value, rc, msg)
    torch.cuda.synchronize()                                                    # nothing was launched, nothing faulted
    assert fit(*ok)[0] == 0
    torch.cuda.synchronize()
    for bad in (dict(bias_sd=0.0), dict(bias_sd=float("nan")), dict(bias_sd="2"), dict(tol=-1.0), dict(tol=True)):
        with pytest.raises(ValueError, match="fit_bias_temperature"):
            ops.fit_bias_temperature(z, y, **bad)
    with pytest.raises(ValueError, match="fit_bias_temperature"):
        ops.fit_bias_temperature(z.double(), y)
    with pytest.raises(ValueError, match="fit_bias_temperature"):
        ops.fit_bias_temperature(z, y, bias=bias[:2])
    with pytest.raises(RuntimeError, match="too small"):
        ops.fit_bias_temperature(z, y, scratch=scratch[:16])
    wide = torch.zeros(2, 513, device="cuda")
    with pytest.raises(RuntimeError, match="V=513"):
        ops.fit_bias_temperature(wide, torch.zeros(2, dtype=torch.int64, device="cuda"))


# ------------------------------------------------------------------------------------------------------ estimator ----
RNN_CFG = dict(module__embedding_size=16, module__hidden_size=16, module__num_layers=2)
BS = 16


@pytest.fixture(scope="module")
def ds():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(120, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


def make_net(ds, seed=11, **kw):
    from slnlp.net import NeuralNetClassifier
    args = dict(module="model.EncoderDecoderGRUAttn", module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y,
                module__batch_first=True, **RNN_CFG, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1,
                optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05, max_epochs=3, batch_size=BS, device="cuda",
                gradient_clipping={"gradient_clip_value": 0.5}, scoring=["accuracy", "neg_log_loss"])
    args.update(kw)
    net = NeuralNetClassifier(**args)
    torch.manual_seed(seed)
    return net.initialize()


def _sd(net):
    return {k: v.detach().cpu().clone() for k, v in net.module_.state_dict().items()}


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def _strip(history):
    return [{k: v for k, v in r.items() if k != "dur"} for r in history]


def _valid(net, ds):
    return ds[net._train_split(ds)[1]]


def _quiet_fit(net, ds):
    """``partial_fit`` with the "cap" / "pivot" warning, which does not fail a fit, kept out of the way of -W error runs."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return net.partial_fit(ds)


def raw_logp(net, data):
    """The uncalibrated float32 log-probs ``predict_proba`` starts from."""
    hidden = {k: net.__dict__.pop(k) for k in ("calibration_", "temperature_") if k in net.__dict__}
    keep = net.predict_nonlinearity
    net.set_params(predict_nonlinearity="none")
    try:
        return net.predict_proba(data)
    finally:
        net.set_params(predict_nonlinearity=keep)
        net.__dict__.update(hidden)


def _same_calibration(a, b):
    return list(a) == list(b) and all(np.array_equal(a[k], b[k]) if k == "bias" else a[k] == b[k] for k in a)


@pytest.fixture(scope="module")
def off(ds):
    return make_net(ds).partial_fit(ds)


@pytest.fixture(scope="module")
def temp(ds):
    return make_net(ds, calibration=TEMPERATURE).partial_fit(ds)


@pytest.fixture(scope="module")
def on(ds):
    return _quiet_fit(make_net(ds, calibration=BIAS), ds)


def test_the_option_changes_nothing_but_probabilities_and_predictions(ds, off, temp, on):
    assert _strip(on.history) == _strip(off.history) == _strip(temp.history)
    assert _same(_sd(on), _sd(off)) and _same(_sd(temp), _sd(off))
    va = _valid(on, ds)
    assert np.array_equal(raw_logp(on, va), raw_logp(off, va))
    c = on.calibration_
    assert c["method"] == "bias_temperature" and c["bias_sd"] == 2.0 and c["temperature"] == on.temperature_ == 1.0 / c["beta"]
    assert c["rows"] == len(va) and c["bad_labels"] == 0 and c["bias"].shape == (len(on.classes_),)
    assert c["reason"] in ("gradient", "cap") and 1 <= c["iterations"] <= 48
    assert "method" not in temp.calibration_ and not hasattr(temp, "_cal_bias") and not hasattr(off, "calibration_")
    # predict is the arg-max of the calibrated probabilities, consistent with predict_proba and predict_topk
    proba = on.predict_proba(ds)
    assert np.array_equal(on.predict(ds), on.classes_[proba.argmax(axis=1)])
    labels, _ = on.predict_topk(ds, k=1)
    assert np.array_equal(labels[:, 0], on.predict(ds))


def test_bias_is_the_restatements_on_the_valid_log_probs(ds, off, on):
    va = _valid(off, ds)
    z = raw_logp(off, va)
    want = fit_bias_temperature_ref(z, va.y, 2.0, TOL)
    c = on.calibration_
    print(f"device {c['reason']} after {c['iterations']}, beta {c['beta']!r}; restatement {want['reason']} after {want['iterations']}, "
          f"beta {want['beta']!r}")
    # (a fit's own log-probs are not chosen for clear decisions: near the round-off floor of F the two sides may halve differently,
    # which the bounds allow -- they hold for any two points that passed the gradient test; tol covers one that stopped at the cap)
    g_tol = TOL if c["reason"] == "gradient" and want["reason"] == "gradient" else 1e-7
    _held_to_the_restatement("the valid split", z, va.y, 2.0, c, want, tol=g_tol)
    proba = on.predict_proba(va)
    w = torch.softmax(torch.from_numpy(shift_logp_ref(z, c["beta"], c["bias"]).astype(np.float32)), dim=-1).numpy()
    assert np.abs(proba - w).max() <= 1e-6 and np.abs(proba.sum(axis=1) - 1.0).max() <= 1e-6


def test_log_loss_on_the_valid_split_falls_by_what_the_fit_says_and_below_the_temperatures(ds, off, temp, on):
    from sklearn.metrics import log_loss
    va = _valid(on, ds)
    labels = np.arange(len(on.classes_))
    before, t, after = (log_loss(va.y, n.predict_proba(va), labels=labels) for n in (off, temp, on))
    c = on.calibration_
    print(f"valid log-loss {before:.6f} -> temperature {t:.6f}, bias_temperature {after:.6f}; the fit: {c['nll_before']:.6f} -> {c['nll_after']:.6f}")
    assert abs((before - after) - (c["nll_before"] - c["nll_after"])) <= 1e-5      # float32 probabilities against the fit's fp64
    # the penalised optimum is at least as good as (beta_T, 0) in F, whose penalty is 0: nll_after <= F* <= the temperature's
    assert c["nll_after"] + c["penalty"] <= temp.calibration_["nll_after"] + 1e-12
    assert after <= t + 1e-5


def test_save_load_and_warm_start(ds, on, off, tmp_path):
    on.save_params(str(tmp_path / "on"))
    with open(tmp_path / "on" / "calibration.json") as f:
        saved = json.load(f)
    assert saved["method"] == "bias_temperature" and saved["bias"] == on.calibration_["bias"].tolist()
    fresh = make_net(ds, seed=5, calibration=BIAS)
    assert not hasattr(fresh, "temperature_")
    fresh.load_params(str(tmp_path / "on"))
    assert _same_calibration(fresh.calibration_, on.calibration_) and fresh.temperature_ == on.temperature_
    assert np.array_equal(fresh.predict_proba(ds), on.predict_proba(ds))
    plain = make_net(ds, seed=5)                                                # with the option off none is read
    plain.load_params(str(tmp_path / "on"))
    assert not hasattr(plain, "temperature_") and np.array_equal(plain.predict_proba(ds), off.predict_proba(ds))
    net = _quiet_fit(make_net(ds, calibration=BIAS, max_epochs=1), ds)          # warm start: the second fit recalibrates
    first = net.calibration_["bias"].copy()
    _quiet_fit(net, ds)
    va = _valid(net, ds)
    want = fit_bias_temperature_ref(raw_logp(net, va), va.y, 2.0, TOL)
    assert len(net.history) == 2 and not np.array_equal(first, net.calibration_["bias"])
    g_tol = TOL if net.calibration_["reason"] == "gradient" and want["reason"] == "gradient" else 1e-7
    _held_to_the_restatement("warm start", raw_logp(net, va), va.y, 2.0, net.calibration_, want, tol=g_tol)


def test_lockstep_group_matches_solo_fits(ds):
    from slnlp.lockstep import fit_lockstep, predict_proba_lockstep
    settings, lrs = [BIAS, None, TEMPERATURE, {"method": "bias_temperature", "bias_sd": 0.5}], [0.05, 0.02, 0.1, 0.05]
    solo = [_quiet_fit(make_net(ds, seed=20 + f, lr=lr, calibration=s), ds) for f, (lr, s) in enumerate(zip(lrs, settings))]
    lock = [make_net(ds, seed=20 + f, lr=lr, calibration=s) for f, (lr, s) in enumerate(zip(lrs, settings))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        fit_lockstep(lock, [ds] * 4)
    probas = predict_proba_lockstep(lock, [ds] * 4)
    for f, (a, b) in enumerate(zip(solo, lock)):
        assert _strip(a.history) == _strip(b.history) and _same(_sd(a), _sd(b)), f
        ca, cb = getattr(a, "calibration_", None), getattr(b, "calibration_", None)
        assert (ca is None and cb is None) or _same_calibration(ca, cb), f
        assert np.array_equal(probas[f], a.predict_proba(ds)), f
    assert hasattr(lock[0], "_cal_bias") and hasattr(lock[3], "_cal_bias") and not hasattr(lock[2], "_cal_bias") and not hasattr(lock[1], "temperature_")
    assert lock[3].calibration_["bias_sd"] == 0.5 and not np.array_equal(lock[3].calibration_["bias"], lock[0].calibration_["bias"])


# ------------------------------------------------------------------------------------------------------ consumers ----
class _Shifted:
    """A judge over a member's log-probs shifted by ``ops.shift_logp`` BEFOREHAND: what every consumer of a bias-calibrated fit must
    equal.  It is the member with its calibration taken away and the shift put into its forward hook."""

    def __init__(self, net):
        import copy
        from slnlp import ops
        self.net = copy.copy(net)
        bias, state = net._cal_bias, net._cal_state
        for k in ("calibration_", "temperature_", "_cal_state", "_cal_bias", "conformal_", "_conf_state", "rejection_", "_rej_state"):
            self.net.__dict__.pop(k, None)
        inner = net._forward_logp

        def forward(ds, then):
            def shifted(logp, yd):
                logp = logp if logp.dtype == torch.float32 else logp.float()
                return then(ops.shift_logp(logp, bias, state=state, out=logp), yd)
            return inner(ds, shifted)
        self.net._forward_logp = forward


def _judged(judge, ds, calibrated=True):
    """Every report the issue names, from one judge; arrays and dicts as they come."""
    judge.conformalize(ds, alpha=0.2, method="aps", seed=3, calibrated=calibrated)
    rel = judge.reliability(ds, bins=10, calibrated=calibrated)
    rank = judge.ranking(ds, calibrated=calibrated)
    risk = judge.risk_coverage(ds, calibrated=calibrated)
    errors = judge.error_analysis(ds, pairs=5, top_k=2, calibrated=calibrated)
    interval = judge.score_interval(ds, scoring=["accuracy", "neg_log_loss"], replicates=50, seed=1, calibrated=calibrated)
    return {"reliability": {k: rel[k] for k in ("ece", "mce", "brier", "nll", "accuracy", "confidence")},
            "ranking": {k: rank[k] for k in ("auc_macro", "ap_macro", "auc", "ap")},
            "topk": judge.predict_topk(ds, k=3, calibrated=calibrated),
            "qhat": judge.conformal_["qhat"], "sets": judge.predict_set(ds, return_mask=True),
            "risk": {k: risk[k] for k in ("aurc", "e_aurc", "errors", "coverage_at_risk", "risk_at_coverage")},
            "errors": {k: errors[k] for k in ("confusion", "accuracy", "pairs", "topk")},
            "interval": {k: interval[k] for k in ("accuracy", "neg_log_loss")}}


def _equal(a, b):
    if a is None or isinstance(a, (str, bool)):
        return type(a) is type(b) and a == b
    if isinstance(a, dict):
        return list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_every_consumer_of_a_net_equals_the_same_call_on_shifted_log_probs(ds, on):
    got, want = _judged(on, ds), _judged(_Shifted(on).net, ds, calibrated=False)
    assert _equal(got, want), {k: _equal(got[k], want[k]) for k in got}
    rel = on.reliability(ds)
    assert rel["calibration"] == "bias_temperature" and rel["temperature"] == on.temperature_
    assert on.ranking(ds)["calibration"] == on.risk_coverage(ds)["calibration"] == "bias_temperature"
    assert on.error_analysis(ds)["calibration"] == on.score_interval(ds, scoring="accuracy", replicates=8)["calibration"] == "bias_temperature"
    raw = on.reliability(ds, calibrated=False)
    assert "calibration" not in raw and raw["temperature"] == 1.0 and raw["nll"] != rel["nll"]
    on._set_conformal(None)
    on._set_rejection(None)


def test_wrappers_holding_such_a_member_equal_the_same_calls_on_shifted_log_probs(ds, on, temp):
    from slnlp import OutOfFold, PriorShift, VotingEnsemble
    shifted = _Shifted(on).net
    # an ensemble of the bias member and a temperature member: the first enters shifted at beta = 1, the second at its own beta
    got = _judged(VotingEnsemble([on, temp]), ds)
    want = _judged(VotingEnsemble([shifted, temp]), ds)
    assert _equal(got, want), {k: _equal(got[k], want[k]) for k in got}
    assert "calibration" not in VotingEnsemble([on, temp]).reliability(ds)
    assert not _equal(got["reliability"], _judged(VotingEnsemble([on, temp], calibrated=False), ds)["reliability"])
    V = len(on.classes_)
    source = np.full(V, 1.0 / V)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a, b = PriorShift(on, source).fit(ds), PriorShift(shifted, source, calibrated=False).fit(ds)
    assert np.array_equal(a.priors_, b.priors_) and a.prior_shift_["iterations"] == b.prior_shift_["iterations"]
    got, want = _judged(a, ds), _judged(b, ds)
    assert _equal(got, want), {k: _equal(got[k], want[k]) for k in got}
    half = len(ds) // 2
    folds = [np.arange(half), np.arange(half, len(ds))]
    got, want = _judged(OutOfFold([on, temp], folds, dataset=ds), ds), _judged(OutOfFold([shifted, temp], folds, dataset=ds), ds)
    assert _equal(got, want), {k: _equal(got[k], want[k]) for k in got}
