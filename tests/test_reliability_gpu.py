"""GPU: reliability diagnostics on the device -- ``slnlp_reliability_rows`` through the C ABI against the numpy restatement
(tests/reliability_ref.py, itself held to a direct fp64 softmax on the CPU), the scoring names in a fit's history, in lockstep
groups and in the grid search, and ``NeuralNetClassifier.reliability``.

The bounds: conf, brier and nll of a row agree with the restatement to 1e-9 (absolute; relative for an nll above 1) -- the bound
the calibration parity tests hold the same fp64 arithmetic to; the row codes are EXACTLY the bin rule applied to the downloaded
conf, and the table is BIT FOR BIT the restated summation order applied to the downloaded rows; where no reference conf * B lies
within 1e-6 of an inner bin edge, bins agree exactly with the restatement's and ece / mce / brier / nll to 1e-9."""
import json
import os

import numpy as np
import pytest
import torch

from reliability_ref import bin_of, reliability_ref, rows_ref, summary_ref, table_ref
from test_calibration_cpu import make_logp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPERATURE = {"method": "temperature"}
BOUND = 1e-9
SCORES = ("ece", "mce", "brier", "nll", "accuracy", "confidence")


def _device(logp, y, ld=None):
    """``logp`` on the device, its rows ``ld`` floats apart (the padding is NaN: never to be read), and the labels."""
    N, V = logp.shape
    buf = torch.full((N, ld or V), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(logp).cuda()
    return buf[:, :V], torch.from_numpy(np.asarray(y, dtype=np.int64)).cuda()


def _kernel_cases():
    bad = make_logp(33, 7, 2.0, 0.6, 4)
    bad[1][3], bad[1][20] = -1, 7
    nan = make_logp(33, 7, 2.0, 0.6, 5)
    nan[0][5, 2] = np.nan
    hole = make_logp(33, 7, 2.0, 0.6, 6)
    hole[0][7, (hole[1][7] + 1) % 7] = -np.inf
    return [("N1_V2", np.log(np.array([[0.83, 0.17]], dtype=np.float32)), np.array([1]), None),
            ("N5_V3", *make_logp(5, 3, 2.0, 0.6, 1), None),
            ("N257_V70_over", *make_logp(257, 70, 8.0, 0.6, 1), None),           # rows wrap a block's four waves, columns the 64 lanes
            ("N257_V70_under", *make_logp(257, 70, 0.3, 0.9, 2), None),
            ("N33_V129_ld136", *make_logp(33, 129, 4.0, 0.6, 3), 136),
            ("N300_V202", *make_logp(300, 202, 3.0, 0.5, 2), None),               # more rows than the table's 256 threads
            ("two_bad_labels", *bad, None), ("one_nan_row", *nan, None), ("one_minus_inf_column", *hole, None)]


def _clear_of_inner_edges(ref_rows, bins):
    """No scored row's reference conf * B within 1e-6 of an integer strictly between 0 and B: a row that could hop bins cannot
    hide behind a tolerance (the top edge is harmless: the bins are closed on the right)."""
    t = ref_rows[ref_rows[:, 3] >= 0, 0] * bins
    near = np.round(t)
    return not np.any((np.abs(t - near) <= 1e-6) & (near > 0) & (near < bins))


def _same_or_both_nan(a, b, tol=0.0):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


# ------------------------------------------------------------------------------------------------- kernels, C ABI ----
def test_kernel_against_the_restatement():
    from slnlp import ops
    worst = {"conf": 0.0, "brier": 0.0, "nll": 0.0, "scores": 0.0}
    calls = saturated = 0
    for name, logp, y, ld in _kernel_cases():
        z, yd = _device(logp, y, ld)
        for beta in (None, 0.16, 6.25):
            state = None if beta is None else ops.temperature_state(beta, "cuda")
            for bins in (1, 10, 15, 64):
                out = ops.reliability_rows(z, yd, bins=bins, state=state)
                rows, table = out[0].cpu().numpy(), out[1].cpu().numpy()
                want = rows_ref(logp, y, bins, 1.0 if beta is None else beta)
                tag = (name, beta, bins)
                assert rows.shape == (len(y), 4) and table.shape == (bins + 1, 4), tag
                # the per-row terms
                scored = want[:, 3] >= 0
                assert np.array_equal(rows[~scored], want[~scored], equal_nan=True), tag   # (0, 0, 0, -1) and (NaN, NaN, NaN, -2)
                assert np.array_equal(rows[:, 3] >= 0, scored), tag
                d = np.abs(rows[scored, :3] - want[scored, :3])
                d[:, 2] /= np.maximum(1.0, np.abs(want[scored, 2]))
                assert np.isfinite(d).all() and d.max(initial=0.0) <= BOUND, (tag, d.max(axis=0))
                for k, col in enumerate(("conf", "brier", "nll")):
                    worst[col] = max(worst[col], float(d[:, k].max(initial=0.0)))
                # exactness from the downloaded rows: the code is the bin of the STORED conf and the arg-max's verdict ...
                correct = logp.argmax(axis=1) == y
                assert np.array_equal(rows[scored, 3], 2.0 * bin_of(rows[scored, 0], bins) + correct[scored]), tag
                # ... and the table is the restated summation order applied to them, bit for bit
                assert table.tobytes() == table_ref(rows, bins).tobytes(), tag
                # against the restatement alone
                assert _clear_of_inner_edges(want, bins), tag
                assert np.array_equal(rows[:, 3], want[:, 3]), tag
                got, ref = ops.reliability_download(out), summary_ref(table_ref(want, bins))
                assert (got["rows"], got["bad_labels"], got["nan_rows"]) == (ref["rows"], ref["bad_labels"], ref["nan_rows"]), tag
                for k in SCORES:
                    assert _same_or_both_nan(got[k], ref[k], BOUND * max(1.0, abs(ref[k]))), (tag, k, got[k], ref[k])
                    if not np.isnan(ref[k]):
                        worst["scores"] = max(worst["scores"], abs(got[k] - ref[k]) / max(1.0, abs(ref[k])))
                assert np.array_equal(got["bins"]["count"], table_ref(want, bins)[:bins, 0].astype(np.int64)), tag
                calls += 1
                saturated += int((rows[scored, 0] == 1.0).sum())
        if name == "one_nan_row":
            assert got["nan_rows"] == 1 and all(np.isnan(got[k]) for k in ("ece", "mce", "brier", "nll")) and np.isfinite(got["accuracy"])
        if name == "two_bad_labels":
            assert got["bad_labels"] == 2 and got["rows"] == 31
    assert saturated > 0, "the overconfident family holds rows whose confidence is exactly 1"
    print(f"{calls} calls; max |device - restatement|: {worst}")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "reliability_parity.json"), "w") as f:
        json.dump({"test": "tests/test_reliability_gpu.py::test_kernel_against_the_restatement", "device": torch.cuda.get_device_name(0),
                   "bound": BOUND, "calls": calls, "max_abs_conf": worst["conf"], "max_abs_brier": worst["brier"],
                   "max_nll_abs_or_relative_above_1": worst["nll"], "max_scores_abs_or_relative_above_1": worst["scores"],
                   "cases": [c[0] for c in _kernel_cases()], "bins": [1, 10, 15, 64], "beta": [None, 0.16, 6.25]}, f, indent=1)
        f.write("\n")


def test_the_result_is_a_pure_function_of_the_arguments():
    from slnlp import ops
    z, y = _device(*make_logp(300, 202, 3.0, 0.5, 2))
    state = ops.temperature_state(0.16, "cuda")
    out = ops.reliability_buffers(300, 15, "cuda")
    assert out[0]._base is out[1]._base and out[1].data_ptr() == out[0].data_ptr() + 300 * 32     # slices of one allocation
    first = ops.reliability_rows(z, y, state=state, out=out)
    assert first is out
    a = out[0]._base.cpu().numpy().tobytes()
    assert ops.reliability_rows(z, y, state=state, out=out)[0]._base.cpu().numpy().tobytes() == a       # over its own leftovers
    other = (torch.full((300, 4), float("nan"), dtype=torch.float64, device="cuda"), torch.full((16, 4), 7.0, dtype=torch.float64, device="cuda"))
    ops.reliability_rows(z, y, state=state, out=other)
    assert other[0].cpu().numpy().tobytes() + other[1].cpu().numpy().tobytes() == a
    fresh = ops.reliability_rows(z, y, state=state)
    assert fresh[0]._base.cpu().numpy().tobytes() == a
    # beta = 1 from a state and beta = 1 as the null pointer: the same bits
    one = ops.reliability_rows(z, y, state=ops.temperature_state(1.0, "cuda"))
    assert one[0]._base.cpu().numpy().tobytes() == ops.reliability_rows(z, y)[0]._base.cpu().numpy().tobytes() != a


def test_download_is_one_copy(monkeypatch):
    from slnlp import ops
    out = ops.reliability_rows(*_device(*make_logp(257, 70, 8.0, 0.6, 1)), bins=10)
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(tuple(t.shape)) or real(t, *a, **k))
    got = ops.reliability_download(out)
    monkeypatch.undo()
    assert copies == [(11, 4)], copies
    assert set(got) == {"ece", "mce", "brier", "nll", "accuracy", "confidence", "rows", "bad_labels", "nan_rows", "bins"}
    assert set(got["bins"]) == {"count", "confidence", "accuracy"} and all(len(v) == 10 for v in got["bins"].values())
    assert got["bins"]["count"].sum() == got["rows"] == 257


def test_bad_arguments_return_codes_and_messages():
    from slnlp import _lib, ops
    lib = _lib.load()
    z, y = _device(*make_logp(5, 3, 2.0, 0.6, 1))
    state = ops.temperature_state(0.5, "cuda")
    rows, table = ops.reliability_buffers(5, 15, "cuda")
    p, st = _lib.ptr, _lib.stream_ptr()
    call = lambda *a: (lib.slnlp_reliability_rows(*a, st), lib.slnlp_last_error().decode())
    good = (p(z), 3, p(y), 5, 3, 15, p(state), p(rows), p(table))
    for i, value, text in [(0, None, "null pointer"), (2, None, "null pointer"), (7, None, "null pointer"), (8, None, "null pointer"),
                           (3, 0, "N=0"), (3, 2 ** 31, "N=2147483648"), (4, 0, "V=0"), (4, 2 ** 31, "V=2147483648"), (1, 2, "ld=2 is less than V=3"),
                           (1, 2 ** 62, "is no addressable matrix"),
                           (5, 0, "bins=0"), (5, 65, "bins=65"), (0, p(z) + 2, "misaligned"), (2, p(y) + 4, "misaligned"),
                           (6, p(state) + 4, "misaligned"), (7, p(rows) + 8, "32-byte aligned"), (8, p(table) + 16, "32-byte aligned"),
                           (7, p(table), "rows and table overlap"), (8, p(rows) + 128, "rows and table overlap"),
                           (7, p(state), "output rows overlaps input beta"), (8, p(state), "output table overlaps input beta")]:
        args = list(good)
        args[i] = value
        rc, msg = call(*args)
        assert rc == 1 and text in msg, (i, value, rc, msg)
    # an output over an input (the buffers are reinterpreted, nothing is launched)
    big = torch.zeros(64, dtype=torch.float64, device="cuda")
    for i, src, text in [(0, big, "output rows overlaps input logp"), (2, big, "output rows overlaps input y")]:
        args = list(good)
        args[i], args[7] = p(src), p(src)
        rc, msg = call(*args)
        assert rc == 1 and text in msg, (i, rc, msg)
    rc, msg = call(*good[:6], None, *good[7:])                                   # beta may be null: beta = 1
    assert rc == 0, msg
    torch.cuda.synchronize()                                                    # no sticky error: nothing faulted
    assert lib.slnlp_abi_version() == 1
    for bins in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="bins"):
            ops.reliability_rows(z, y, bins=bins)
    with pytest.raises(ValueError, match="reliability_rows"):
        ops.reliability_rows(z.double(), y)
    with pytest.raises(ValueError, match="reliability_rows"):
        ops.reliability_rows(z, y.int())
    with pytest.raises(ValueError, match="reliability_rows"):
        ops.reliability_rows(z, y, state=state[:8])
    with pytest.raises(ValueError, match="reliability_rows"):
        ops.reliability_rows(z, y, out=(rows, table[:10]))


# ------------------------------------------------------------------------------------------------------ estimator ----
from test_calibration_gpu import BS, EMA, RNN_CFG, _same, _sd, _strip, make_net, raw_logp  # noqa: E402

NAMES = ["neg_ece", "neg_brier", "accuracy"]


@pytest.fixture(scope="module")
def ds():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(120, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


def _fit_and_watch(net, ds):
    """``net.partial_fit(ds)``, with every epoch's (split, log-probs, labels) that went to ``metrics.epoch_scores`` kept."""
    from slnlp import metrics
    seen, real = [], metrics.epoch_scores

    def watch(names, logp, y, *a, **k):
        seen.append((k.get("split"), logp.detach().cpu().numpy().copy(), y.detach().cpu().numpy().copy()))
        return real(names, logp, y, *a, **k)
    metrics.epoch_scores = watch
    try:
        net.partial_fit(ds)
    finally:
        metrics.epoch_scores = real
    return seen


@pytest.fixture(scope="module")
def plain(ds):
    return make_net(ds, scoring=["accuracy"], calibration=TEMPERATURE).partial_fit(ds)


@pytest.fixture(scope="module")
def scored(ds):
    net = make_net(ds, scoring=NAMES, calibration=TEMPERATURE)
    return net, _fit_and_watch(net, ds)


def _check_reliability(net, data, beta, **kw):
    """``net.reliability(data)`` against the restatement on the log-probs ``predict_proba`` starts from."""
    z = raw_logp(net, data)
    for bins in (4, 15):
        got = net.reliability(data, bins=bins, **kw)
        want_rows = rows_ref(z, data.y, bins, beta)
        assert _clear_of_inner_edges(want_rows, bins)
        want = summary_ref(table_ref(want_rows, bins))
        for k in SCORES:
            assert abs(got[k] - want[k]) <= BOUND * max(1.0, abs(want[k])), (bins, k, got[k], want[k])
        assert (got["rows"], got["bad_labels"], got["nan_rows"]) == (len(data), 0, 0)
        assert np.array_equal(got["bins"]["count"], table_ref(want_rows, bins)[:bins, 0].astype(np.int64))
    return got


def test_history_columns_are_the_restatements_on_the_epoch_log_probs(ds, scored):
    net, seen = scored
    assert len(net.history) == 3 and [s[0] for s in seen] == ["train", "valid"] * 3
    for e, row in enumerate(net.history):
        for split, logp, y in seen[2 * e:2 * e + 2]:
            want_rows = rows_ref(logp, y, 15)
            assert _clear_of_inner_edges(want_rows, 15)
            want = summary_ref(table_ref(want_rows, 15))
            print(f"epoch {e + 1} {split}: ece {-row[f'{split}_neg_ece']:.6f} brier {-row[f'{split}_neg_brier']:.6f}")
            assert abs(row[f"{split}_neg_ece"] + want["ece"]) <= BOUND and abs(row[f"{split}_neg_brier"] + want["brier"]) <= BOUND
            assert row[f"{split}_accuracy"] == want["accuracy"]
            assert row[f"{split}_neg_ece"] <= 0.0 and row[f"{split}_neg_brier"] <= 0.0


def test_the_names_change_nothing_else(ds, plain, scored):
    net = scored[0]
    new = {f"{sp}_{n}" for sp in ("train", "valid") for n in ("neg_ece", "neg_brier")}
    assert all(new <= set(r) for r in net.history) and not any(new & set(r) for r in plain.history)
    drop = lambda hist: [{k: v for k, v in r.items() if k not in new} for r in _strip(hist)]
    assert drop(net.history) == _strip(plain.history)
    assert _same(_sd(net), _sd(plain)) and np.array_equal(net.predict(ds), plain.predict(ds))
    assert np.array_equal(net.predict_proba(ds), plain.predict_proba(ds)) and net.calibration_ == plain.calibration_


def test_labels_outside_the_classes_raise_the_existing_error(ds):
    from slnlp import metrics
    logp, y = _device(*make_logp(33, 7, 2.0, 0.6, 4))
    y[4] = 7
    for names in (["neg_ece"], ["accuracy", "neg_brier"]):
        with pytest.raises(ValueError, match="scoring the valid data: 1 of 33 labels lie outside the 7 classes"):
            metrics.epoch_scores(names, logp, y, split="valid")


def test_reliability_of_a_calibrated_fit(ds, plain, scored):
    net = scored[0]
    assert net.temperature_ != 1.0
    on = _check_reliability(net, ds, net.calibration_["beta"])
    assert on["temperature"] == net.temperature_
    off = _check_reliability(net, ds, 1.0, calibrated=False)
    assert off["temperature"] == 1.0 and off["accuracy"] == on["accuracy"]       # the arg-max never moves
    assert off["nll"] != on["nll"]
    # the same weights without a calibration: calibrated=True has nothing to apply
    hidden = {k: plain.__dict__.pop(k) for k in ("calibration_", "temperature_")}
    try:
        bare = plain.reliability(ds)
    finally:
        plain.__dict__.update(hidden)
    for k, v in off.items():
        assert np.array_equal(v["count"], bare[k]["count"]) if k == "bins" else v == bare[k], k
    assert _same(_sd(net), _sd(plain))
    # y given apart from the dataset, and what is rejected
    assert net.reliability(ds, y=ds.y)["ece"] == on["ece"]
    for bins in (0, 65, 1.5, True, None):
        with pytest.raises(ValueError, match="bins"):
            net.reliability(ds, bins=bins)
    wrong = ds.y.copy()
    wrong[3] = len(net.classes_)
    with pytest.raises(ValueError, match="1 of 120 labels lie outside the"):
        net.reliability(ds, y=wrong)
    with pytest.raises(ValueError, match="shape"):
        net.reliability(ds, y=ds.y[:5])


def test_reliability_of_an_uncalibrated_fit_and_with_ema_weights(ds):
    net = make_net(ds, scoring=NAMES).partial_fit(ds)
    assert _check_reliability(net, ds, 1.0)["temperature"] == 1.0
    ema = make_net(ds, weight_averaging=EMA, calibration=TEMPERATURE).partial_fit(ds)
    before = _sd(ema)
    live = make_net(ds, seed=3)
    live.module_.load_state_dict(ema.module_.state_dict())
    assert not np.array_equal(raw_logp(ema, ds), raw_logp(live, ds)), "predictions come from the averaged weights"
    _check_reliability(ema, ds, ema.calibration_["beta"])
    assert _same(_sd(ema), before), "the live weights came back bit for bit"


def test_reliability_of_a_gru_fit(ds):
    net = make_net(ds, module="model.EncoderDecoderGRUAttn", cfg=RNN_CFG, scoring=NAMES, calibration=TEMPERATURE).partial_fit(ds)
    assert all("valid_neg_ece" in r and "train_neg_brier" in r for r in net.history)
    _check_reliability(net, ds, net.calibration_["beta"])


def test_reliability_of_a_torch_stepped_fit(ds):
    net = make_net(ds, optimizer="torch.optim.RMSprop", lr=1e-3, scoring=NAMES, calibration=TEMPERATURE)
    assert not net._fused
    net.partial_fit(ds)
    assert all(np.isfinite(r["valid_neg_ece"]) and np.isfinite(r["train_neg_brier"]) for r in net.history)
    _check_reliability(net, ds, net.calibration_["beta"])


def test_predict_proba_is_the_manual_forward_loop(ds, plain):
    net = plain
    hidden = {k: net.__dict__.pop(k) for k in ("calibration_", "temperature_")}
    try:
        proba = net.predict_proba(ds)
    finally:
        net.__dict__.update(hidden)
    net.module_.eval()
    with torch.cuda.stream(net._stream), torch.no_grad():
        X, L, y = net._device_data(ds)
        outs = [net.module_(X=X[i:i + BS], y=y[i:i + BS], lengths=L[i:i + BS]) for i in range(0, len(ds), BS)]
        logp = torch.cat(outs)
    torch.cuda.synchronize()
    assert np.array_equal(proba, torch.softmax(logp.cpu(), dim=-1).numpy())
    assert np.array_equal(raw_logp(net, ds), logp.cpu().numpy())


# ------------------------------------------------------------------------------------------------------- lockstep ----
def test_lockstep_group_matches_solo_fits(ds):
    from slnlp.lockstep import fit_lockstep
    lrs = [0.05, 0.02]
    solo = [make_net(ds, seed=20 + f, lr=lr, scoring=NAMES).partial_fit(ds) for f, lr in enumerate(lrs)]
    lock = [make_net(ds, seed=20 + f, lr=lr, scoring=NAMES) for f, lr in enumerate(lrs)]
    fit_lockstep(lock, [ds] * 2)
    for f, (a, b) in enumerate(zip(solo, lock)):
        assert all("train_neg_ece" in r and "valid_neg_brier" in r for r in b.history), f
        assert _strip(a.history) == _strip(b.history) and _same(_sd(a), _sd(b)), f
        ra, rb = a.reliability(ds), b.reliability(ds)
        assert all(ra[k] == rb[k] for k in SCORES) and np.array_equal(ra["bins"]["count"], rb["bins"]["count"]), f


# ----------------------------------------------------------------------------------------------------------- grid ----
def test_sharded_grid_ranks_on_neg_ece(ds):
    from slnlp.grid import ShardedGridSearchCV
    grid = {"lr": [0.05, 0.02]}
    search = lambda width: ShardedGridSearchCV(lambda: make_net(ds, use_graph=False), grid, cv=2, scoring="neg_ece", refit=False,
                                               device="cuda:0", lockstep=width).fit(ds)
    together, one_at_a_time = search(4), search(1)
    assert together.n_units_ == 1 and one_at_a_time.n_units_ == 4
    for k in ("split0_test_score", "split1_test_score", "mean_test_score"):
        a, b = np.asarray(together.cv_results_[k]), np.asarray(one_at_a_time.cv_results_[k])
        print(k, a, b)
        assert np.isfinite(a).all() and (a <= 0.0).all() and np.array_equal(a, b), k
    assert together.best_index_ == int(np.argmax(together.cv_results_["mean_test_score"]))
