"""GPU: temperature calibration fitted on the device -- ``slnlp_fit_temperature`` / ``slnlp_scale_logp`` through the C ABI against
the numpy restatement (tests/calibration_ref.py, itself held to scipy on the CPU), and the estimator option on the solo path,
in lockstep groups and in the grid search.

The bounds (why they hold is written where they are used): a converged fit's temperature agrees with the restatement's to 1e-9
relative and its Newton-step residual is at most 1e-9; ``nll_before`` / ``nll_after`` agree to 1e-12 relative; the calibrated
log-probs lie within one float32 ulp of the fp64 restatement."""
import json
import os

import numpy as np
import pytest
import torch

from calibration_ref import fit_temperature_ref, newton_step, scale_logp_ref
from test_calibration_cpu import make_logp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPERATURE = {"method": "temperature"}


def _device(logp, y, ld=None):
    """``logp`` on the device, its rows ``ld`` floats apart (the padding is NaN: never to be read), and the labels."""
    N, V = logp.shape
    buf = torch.full((N, ld or V), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(logp).cuda()
    return buf[:, :V], torch.from_numpy(np.asarray(y, dtype=np.int64)).cuda()


def _kernel_cases():
    two = np.log(np.array([[0.9, 0.1]], dtype=np.float32))
    bad = make_logp(33, 7, 2.0, 0.6, 4)
    bad[1][3], bad[1][20] = -1, 7
    return [("N1_V2_bound_hi", two, np.array([1]), None), ("N1_V2_bound_lo", two, np.array([0]), None),
            ("N5_V3", *make_logp(5, 3, 2.0, 0.6, 1), None),
            ("N257_V70_over", *make_logp(257, 70, 8.0, 0.6, 1), None), ("N257_V70_under", *make_logp(257, 70, 0.3, 0.9, 2), None),
            ("N33_V129_ld136", *make_logp(33, 129, 4.0, 0.6, 3), 136),
            ("flat", np.full((9, 4), np.log(0.25), dtype=np.float32), np.arange(9) % 4, None),
            ("two_bad_labels", *bad, None)]


# ------------------------------------------------------------------------------------------------- kernels, C ABI ----
def test_fit_temperature_against_the_restatement():
    from slnlp import ops
    worst = {"newton_step_residual": 0.0, "temperature_relative_deviation": 0.0, "cases": {}}
    for name, logp, y, ld in _kernel_cases():
        want = fit_temperature_ref(logp, y)
        got = ops.temperature_download(ops.fit_temperature(*_device(logp, y, ld)))
        print(f"[{name}] device {got}\n{' ' * (len(name) + 3)}ref    {want}")
        assert (got["reason"], got["rows"], got["bad_labels"]) == (want["reason"], want["rows"], want["bad_labels"]), name
        assert got["temperature"] == 1.0 / got["beta"], name
        rec = {"reason": got["reason"], "iterations": got["iterations"], "temperature": got["temperature"]}
        if got["reason"] in ("gradient", "step"):
            # both sides run the same fp64 algorithm; rounding in g is of order V 2^-53 |z| and a converged step is below
            # 2^-40 ~ 1e-12, so 1e-9 leaves three orders of room
            rec["newton_step_residual"] = newton_step(logp, y, got["beta"])
            rec["temperature_relative_deviation"] = abs(got["temperature"] / want["temperature"] - 1.0)
            assert rec["newton_step_residual"] <= 1e-9 and rec["temperature_relative_deviation"] <= 1e-9, (name, rec)
            # the 2^-44 gradient test can fire one evaluation earlier or later
            assert abs(got["iterations"] - want["iterations"]) <= 1 and 1 <= got["iterations"] <= 16, name
            for k in ("newton_step_residual", "temperature_relative_deviation"):
                worst[k] = max(worst[k], rec[k])
        else:
            assert got["beta"] == want["beta"] and got["iterations"] == 0, name
        for k in ("nll_before", "nll_after"):
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (name, k, got[k], want[k])
        assert got["nll_after"] <= got["nll_before"], name
        worst["cases"][name] = rec
    reasons = {r["reason"] for r in worst["cases"].values()}
    assert {"flat", "bound"} <= reasons and reasons & {"gradient", "step"}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "calibration_parity.json"), "w") as f:
        json.dump({"test": "tests/test_calibration_gpu.py::test_fit_temperature_against_the_restatement",
                   "device": torch.cuda.get_device_name(0), "bound": 1e-9, **worst}, f, indent=1)
        f.write("\n")


def test_the_result_is_a_pure_function_of_the_arguments():
    from slnlp import ops
    logp, y = _device(*make_logp(257, 70, 8.0, 0.6, 1))
    state, scratch = torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros(4 * 257, dtype=torch.float64, device="cuda")
    first = ops.fit_temperature(logp, y, state=state, scratch=scratch).cpu().numpy().tobytes()
    assert ops.fit_temperature(logp, y, state=state, scratch=scratch).cpu().numpy().tobytes() == first      # over its own leftovers
    other = ops.fit_temperature(logp, y, state=torch.full((16,), float("nan"), dtype=torch.float64, device="cuda"),
                                scratch=torch.full((4 * 257 + 64,), 7.0, dtype=torch.float64, device="cuda"))
    assert other.cpu().numpy().tobytes() == first
    assert ops.fit_temperature(logp, y).cpu().numpy().tobytes() == first


@pytest.mark.parametrize("N,V,ld,ld_out,beta", [(1, 2, None, None, 64.0), (5, 3, None, None, 0.37), (257, 70, None, 72, 1.0 / 6.25),
                                                (33, 129, 136, 131, 7.5)])
def test_scale_logp(N, V, ld, ld_out, beta):
    from slnlp import ops
    logp = make_logp(N, V, 4.0, 0.6, 5)[0]
    z, _ = _device(logp, np.zeros(N), ld)
    state = ops.temperature_state(beta, "cuda")
    out = torch.full((N, ld_out or V), float("nan"), dtype=torch.float32, device="cuda")[:, :V]
    assert ops.scale_logp(z, state, out=out) is out
    got = out.cpu().numpy()
    want = scale_logp_ref(logp, beta)
    w32 = want.astype(np.float32)
    # fp64 throughout, rounded once: the library's exp / log differ from numpy's far below a float32 ulp, and the ulp covers a
    # value that sits on a rounding boundary
    err = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(w32)).astype(np.float64)
    print(f"[{N} x {V}, beta {beta}] max |device - fp64| = {err.max():.3f} float32 ulp; bits differ from the rounded reference in "
          f"{int((got != w32).sum())} of {got.size}")
    assert err.max() <= 1.0
    assert np.array_equal(got.argmax(axis=1), logp.argmax(axis=1))
    assert torch.equal(ops.scale_logp(z, state), out)                           # a new tensor: the same bits
    same = z.clone() if ld is None else z                                       # in place, over padded rows too
    assert ops.scale_logp(same, state, out=same) is same and torch.equal(same, out)
    if ld is not None:
        assert bool(torch.isnan(same._base[:, V:]).all()), "the padding was never written"


def test_bad_arguments_return_codes_and_messages():
    from slnlp import _lib, ops
    lib = _lib.load()
    z, y = _device(*make_logp(5, 3, 2.0, 0.6, 1))
    state, scratch = torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros(20, dtype=torch.float64, device="cuda")
    p, st = _lib.ptr, _lib.stream_ptr()
    fit = lambda *a: (lib.slnlp_fit_temperature(*a, st), lib.slnlp_last_error().decode())
    assert lib.slnlp_fit_temperature_scratch_bytes(5) == 160 and scratch.numel() * 8 == 160
    assert lib.slnlp_fit_temperature_scratch_bytes(0) == -1 and "N=0" in lib.slnlp_last_error().decode()
    for args, text in [((None, 3, p(y), 5, 3, p(state), p(scratch), 160), "null pointer"),
                       ((p(z), 3, p(y), 5, 3, None, p(scratch), 160), "null pointer"),
                       ((p(z), 2, p(y), 5, 3, p(state), p(scratch), 160), "ld=2 is less than V=3"),
                       ((p(z), 3, p(y), 5, 3, p(state), p(scratch), 159), "too small"),
                       ((p(z), 3, p(y), 5, 3, p(state), p(scratch) + 8, 160), "aligned"),
                       ((p(z), 3, p(y), 0, 3, p(state), p(scratch), 160), "N=0"),
                       ((p(z), 3, p(y), 5, 2 ** 31, p(state), p(scratch), 160), "V=2147483648"),
                       ((p(z), 3, p(y), 5, 3, p(scratch), p(scratch), 160), "overlaps")]:
        rc, msg = fit(*args)
        assert rc == 1 and text in msg, (args, rc, msg)
    scale = lambda *a: (lib.slnlp_scale_logp(*a, st), lib.slnlp_last_error().decode())
    out = torch.zeros(5, 3, device="cuda")
    for args, text in [((None, 3, 5, 3, p(state), p(out), 3), "null pointer"), ((p(z), 3, 5, 3, None, p(out), 3), "null pointer"),
                       ((p(z), 3, 5, 3, p(state), p(out), 2), "less than V=3"),
                       ((p(z), 3, 5, 3, p(state), p(z) + 4, 3), "overlaps logp"),          # shifted by one float: partial overlap
                       ((p(z), 4, 4, 3, p(state), p(z), 3), "overlaps logp")]:             # the same pointer, another stride
        rc, msg = scale(*args)
        assert rc == 1 and text in msg, (args, rc, msg)
    torch.cuda.synchronize()                                                    # nothing was launched, nothing faulted
    with pytest.raises(ValueError, match="fit_temperature"):
        ops.fit_temperature(z.double(), y)
    with pytest.raises(ValueError, match="fit_temperature"):
        ops.fit_temperature(z, y.int())
    with pytest.raises(ValueError, match="scale_logp"):
        ops.scale_logp(z, state[:8])
    with pytest.raises(RuntimeError, match="too small"):
        ops.fit_temperature(z, y, scratch=scratch[:16])


# ------------------------------------------------------------------------------------------------------ estimator ----
CFG = dict(module__embedding_size=32, module__num_heads=4, module__num_layers=1, module__hidden_size=64)
RNN_CFG = dict(module__embedding_size=16, module__hidden_size=16, module__num_layers=2)
BS = 16
EMA = {"kind": "ema", "every": "batch"}


@pytest.fixture(scope="module")
def ds():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(120, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


def make_net(ds, seed=11, module="model.Transformer", cfg=CFG, **kw):
    from slnlp.net import NeuralNetClassifier
    args = dict(module=module, module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y, module__batch_first=True,
                **cfg, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1, optimizer="torch.optim.SGD",
                optimizer__momentum=0.9, lr=0.05, max_epochs=3, batch_size=BS, device="cuda",
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


def raw_logp(net, data):
    """The uncalibrated float32 log-probs ``predict_proba`` starts from (under the averaged weights where it predicts with them)."""
    hidden = {k: net.__dict__.pop(k) for k in ("calibration_", "temperature_") if k in net.__dict__}
    keep = net.predict_nonlinearity
    net.set_params(predict_nonlinearity="none")
    try:
        return net.predict_proba(data)
    finally:
        net.set_params(predict_nonlinearity=keep)
        net.__dict__.update(hidden)


def _softmax32(logp64):
    return torch.softmax(torch.from_numpy(logp64.astype(np.float32)), dim=-1).numpy()


@pytest.fixture(scope="module")
def off(ds):
    return make_net(ds).partial_fit(ds)


@pytest.fixture(scope="module")
def on(ds):
    return make_net(ds, calibration=TEMPERATURE).partial_fit(ds)


def test_the_option_changes_nothing_but_the_probabilities(ds, off, on):
    assert _strip(on.history) == _strip(off.history)
    assert _same(_sd(on), _sd(off))
    assert np.array_equal(on.predict(ds), off.predict(ds))
    assert not hasattr(off, "calibration_") and not hasattr(off, "temperature_")
    # (this model reads the label as decoder input and is right on every valid row after three epochs: "bound" is a fair end)
    assert on.calibration_["temperature"] == on.temperature_ and on.calibration_["reason"] in ("gradient", "step", "bound")
    assert on.calibration_["rows"] == len(_valid(on, ds)) and on.calibration_["bad_labels"] == 0


def test_temperature_is_the_restatements_on_the_valid_log_probs(ds, off, on):
    va = _valid(off, ds)
    z = raw_logp(off, va)
    assert np.array_equal(z, raw_logp(on, va))
    want = fit_temperature_ref(z, va.y)
    print(f"T = {on.temperature_!r} (restatement {want['temperature']!r}); {on.calibration_}")
    assert abs(on.temperature_ / want["temperature"] - 1.0) <= 1e-9 and on.calibration_["reason"] == want["reason"]
    proba = on.predict_proba(va)
    assert np.abs(proba - _softmax32(scale_logp_ref(z, 1.0 / on.temperature_))).max() <= 1e-6
    assert np.abs(proba.sum(axis=1) - 1.0).max() <= 1e-6
    assert np.array_equal(proba.argmax(axis=1), off.predict_proba(va).argmax(axis=1))
    # predict_nonlinearity != "auto": the calibrated log-probs themselves
    on.set_params(predict_nonlinearity="none")
    try:
        lp = on.predict_proba(va)
    finally:
        on.set_params(predict_nonlinearity="auto")
    w32 = scale_logp_ref(z, on.calibration_["beta"]).astype(np.float32)
    assert np.abs(lp - w32).max() <= np.spacing(np.abs(w32)).max() and np.array_equal(_softmax32(lp.astype(np.float64)), proba)


def test_log_loss_on_the_valid_split_goes_down_by_what_the_fit_says(ds, off, on):
    from sklearn.metrics import log_loss
    va = _valid(on, ds)
    labels = np.arange(len(on.classes_))
    before, after = log_loss(va.y, off.predict_proba(va), labels=labels), log_loss(va.y, on.predict_proba(va), labels=labels)
    c = on.calibration_
    print(f"valid log-loss {before:.6f} -> {after:.6f}; the fit: {c['nll_before']:.6f} -> {c['nll_after']:.6f}")
    assert after <= before
    assert abs((before - after) - (c["nll_before"] - c["nll_after"])) <= 1e-5


def test_save_and_load(ds, on, off, tmp_path):
    on.save_params(str(tmp_path / "on"))
    with open(tmp_path / "on" / "calibration.json") as f:
        assert json.load(f) == on.calibration_
    fresh = make_net(ds, seed=5, calibration=TEMPERATURE)
    assert not hasattr(fresh, "temperature_")
    fresh.load_params(str(tmp_path / "on"))
    assert fresh.temperature_ == on.temperature_ and fresh.calibration_ == on.calibration_
    assert np.array_equal(fresh.predict_proba(ds), on.predict_proba(ds))
    off.save_params(str(tmp_path / "off"))                                      # without the option no such file is written
    assert "calibration.json" not in os.listdir(tmp_path / "off")
    plain = make_net(ds, seed=5)                                                # ... and with the option off none is read
    plain.load_params(str(tmp_path / "on"))
    assert not hasattr(plain, "temperature_") and np.array_equal(plain.predict_proba(ds), off.predict_proba(ds))


def test_warm_start_recalibrates(ds):
    net = make_net(ds, calibration=TEMPERATURE, max_epochs=1).partial_fit(ds)
    first = net.temperature_
    net.partial_fit(ds)
    va = _valid(net, ds)
    assert len(net.history) == 2 and first is not None
    assert abs(net.temperature_ / fit_temperature_ref(raw_logp(net, va), va.y)["temperature"] - 1.0) <= 1e-9


def test_with_weight_averaging_the_averaged_weights_are_calibrated(ds):
    plain = make_net(ds, weight_averaging=EMA).partial_fit(ds)
    net = make_net(ds, weight_averaging=EMA, calibration=TEMPERATURE).partial_fit(ds)
    assert _same(_sd(net), _sd(plain)), "the live weights are what they are without calibration"
    assert _same({k: v.cpu() for k, v in net.averaged_state_dict().items()}, {k: v.cpu() for k, v in plain.averaged_state_dict().items()})
    va = _valid(net, ds)
    z = raw_logp(plain, va)                                                      # predict: the averaged weights
    live = make_net(ds, seed=3)
    live.module_.load_state_dict(plain.module_.state_dict())
    assert not np.array_equal(z, raw_logp(live, va))
    assert abs(net.temperature_ / fit_temperature_ref(z, va.y)["temperature"] - 1.0) <= 1e-9
    assert _same(_sd(net), _sd(plain))                                           # ... and after predicting, still


def test_gru_fit(ds):
    net = make_net(ds, module="model.EncoderDecoderGRUAttn", cfg=RNN_CFG, calibration=TEMPERATURE).partial_fit(ds)
    va = _valid(net, ds)
    want = fit_temperature_ref(raw_logp(net, va), va.y)
    print(f"GRU: T = {net.temperature_!r} (restatement {want['temperature']!r}), {net.calibration_['reason']}")
    assert net.calibration_["reason"] == want["reason"]
    assert abs(net.temperature_ / want["temperature"] - 1.0) <= 1e-9


# ------------------------------------------------------------------------------------------------------- lockstep ----
def test_lockstep_group_matches_solo_fits(ds):
    from slnlp.lockstep import fit_lockstep, predict_proba_lockstep
    settings, lrs = [TEMPERATURE, None, TEMPERATURE], [0.05, 0.02, 0.1]
    solo = [make_net(ds, seed=20 + f, lr=lr, calibration=s).partial_fit(ds) for f, (lr, s) in enumerate(zip(lrs, settings))]
    lock = [make_net(ds, seed=20 + f, lr=lr, calibration=s) for f, (lr, s) in enumerate(zip(lrs, settings))]
    fit_lockstep(lock, [ds] * 3)
    probas = predict_proba_lockstep(lock, [ds] * 3)
    for f, (a, b) in enumerate(zip(solo, lock)):
        assert _strip(a.history) == _strip(b.history) and _same(_sd(a), _sd(b)), f
        assert getattr(a, "calibration_", None) == getattr(b, "calibration_", None), f
        assert np.array_equal(probas[f], a.predict_proba(ds)), f
    assert hasattr(lock[0], "temperature_") and hasattr(lock[2], "temperature_") and not hasattr(lock[1], "temperature_")
    plain = make_net(ds, seed=21, lr=0.02).partial_fit(ds)                       # the third fit: as if the option did not exist
    assert _same(_sd(plain), _sd(lock[1])) and np.array_equal(probas[1], plain.predict_proba(ds))


# ----------------------------------------------------------------------------------------------------------- grid ----
def test_sharded_grid_with_calibration_as_an_axis(ds, monkeypatch):
    from slnlp import grid as grid_mod, lockstep as lockstep_mod
    from slnlp.grid import ShardedGridSearchCV
    from slnlp.net import ScoringWrapper, _CachedPredictor
    grid = {"calibration": [None, TEMPERATURE]}
    one_at_a_time, seen = [], []
    real_one, real_predict = grid_mod.default_fit_and_score, lockstep_mod.predict_proba_lockstep
    monkeypatch.setattr(grid_mod, "default_fit_and_score", lambda *a, **k: one_at_a_time.append(1) or real_one(*a, **k))

    def predict(nets, tests):
        out = real_predict(nets, tests)
        seen.extend((n.get_params()["calibration"], t, getattr(n, "temperature_", None), raw_logp(n, t), p) for n, t, p in zip(nets, tests, out))
        return out
    monkeypatch.setattr(lockstep_mod, "predict_proba_lockstep", predict)
    gs = ShardedGridSearchCV(lambda: make_net(ds, use_graph=False), grid, cv=2, refit=False, device="cuda:0", lockstep=4).fit(ds)
    assert not one_at_a_time and gs.n_tasks_ == 4 and gs.n_units_ == 1 and len(seen) == 4
    cands, folds, _, _ = grid_mod.build_tasks(grid, ds.y, 2)
    res = gs.cv_results_
    for ci, cand in enumerate(cands):
        for fi, (train_idx, test_idx) in enumerate(folds):
            (setting, test, T, z, proba), = [s for s in seen if s[0] == cand["calibration"] and np.array_equal(s[1].ids, ds[test_idx].ids)]
            assert (T is not None) == (cand["calibration"] is not None)
            want = _softmax32(scale_logp_ref(z, 1.0 / T)) if T is not None else _softmax32(z.astype(np.float64))
            wr = ScoringWrapper("neg_log_loss", ds[train_idx].labels())
            score = float(wr(_CachedPredictor(want, np.arange(want.shape[1])), None, test.y))
            # the device rounds the calibrated log-probs once to float32, within one ulp of the restatement's (2^-20 for |z| < 16),
            # and the float32 softmax adds a few 2^-24 relative: a mean of -log p moves by less than 4e-6
            assert abs(res[f"split{fi}_test_score"][ci] - score) <= (4e-6 if T is not None else 0.0), (ci, fi)
            assert res[f"split{fi}_test_score"][ci] == float(wr(_CachedPredictor(proba, np.arange(want.shape[1])), None, test.y))
        assert abs(res["mean_test_score"][ci] - np.mean([res[f"split{fi}_test_score"][ci] for fi in range(2)])) <= 1e-15
    assert res["mean_test_score"][0] != res["mean_test_score"][1]
