"""GPU: label-shift adaptation on the device -- ``slnlp_fit_priors`` / ``slnlp_shift_logp`` against the numpy restatement
(tests/prior_shift_ref.py, itself checked on the CPU) and ``slnlp.PriorShift`` on a fit and on an ensemble.

The bounds: with ``tol = 0`` (no stop decision) table rows 0 and 1 and the gain agree with the restatement to 64 N 2^-53 relative
plus 2^-60 -- sums of at most N positive terms that differ only in their order, fp64 exp / log that differ by a few ulp, and an
EM that amplifies neither -- and row 2 to that bound times 1 / pi_c; the re-weighted log-probs lie within one float32 ulp of the
fp64 restatement, the standard tests/test_calibration_gpu.py holds ``scale_logp`` to."""
import numpy as np
import pytest
import torch

from prior_shift_ref import (FLOOR, fit_priors, gaussian_shift_problem, iterate_bound, iterate_errors, make_case, shift_logp, ulp_error)

pytestmark = pytest.mark.gpu

# one of each boundary: V in {1, 2, 63, 64, 65, 202} (lanes stride the columns by 64), N in {1, 3, 255, 256, 257, 1025} (the
# 256-thread tree, four rows per block), two with ld = V + 3 and NaN in the padding, beta_dev null and a state with beta = 0.5
CASES = [(1, 1, None, None), (3, 2, None, 0.5), (255, 63, None, None), (256, 64, 67, None), (257, 65, None, 0.5), (1025, 202, 205, 0.5)]


def _device(z, ld=None):
    """``z`` on the device, its rows ``ld`` floats apart (the padding is NaN: never to be read)."""
    N, V = z.shape
    buf = torch.full((N, ld or V), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(z).cuda()
    return buf[:, :V]


def _state(beta):
    from slnlp import ops
    return None if beta is None else ops.temperature_state(beta, "cuda")


def _fit(z, ls, ld=None, beta=None, **kw):
    from slnlp import ops
    return ops.priors_download(ops.fit_priors(_device(z, ld), torch.from_numpy(ls).cuda(), state=_state(beta), **kw))


@pytest.fixture(scope="module")
def cases():
    return {(N, V): make_case(N, V, 100 + N) for N, V, _, _ in CASES}


# ------------------------------------------------------------------------------------------------- kernels, C ABI ----
@pytest.mark.parametrize("N,V,ld,beta", CASES)
def test_iterates_against_the_restatement(cases, N, V, ld, beta):
    z, ls = cases[(N, V)]
    for max_iter in (0, 1, 8):
        want = fit_priors(z, ls, beta=beta or 1.0, max_iter=max_iter, tol=0.0)
        got = _fit(z, ls, ld, beta, max_iter=max_iter, tol=0.0)
        err = iterate_errors(got, want, N)
        print(f"[{N} x {V}, ld {ld}, beta {beta}, max_iter {max_iter}] error / bound: {err}; gain {got['gain']:.6g}, d {got['d']:.3g}")
        assert (got["rows"], got["nan_rows"]) == (N, 0)
        # tol = 0 stops only a run whose priors no longer move at all (V = 1: pi = 1 from the start); otherwise the cap ends it
        if V > 1:
            assert min(want["d_trace"]) > 1e-9
        assert (got["reason"], got["iterations"]) == (want["reason"], want["iterations"])
        assert max(err.values()) <= 1.0, err
        assert abs(got["d"] - want["d"]) <= 2.0 * iterate_bound(1.0, N)      # the difference of two priors, each at most 1
        assert got["gain"] >= -2.0 ** -40 and abs(got["priors"].sum() - 1.0) <= iterate_bound(1.0, N)
        if max_iter == 0:
            assert np.array_equal(got["priors"], got["mean_proba"])
        assert np.array_equal(got["log_ratio"], np.log(np.maximum(got["priors"], FLOOR)) - ls) or \
            np.abs(got["log_ratio"] - (np.log(np.maximum(got["priors"], FLOOR)) - ls)).max() <= 2.0 ** -42     # (device log vs numpy log)


def test_stopping_follows_the_restatement():
    V, N, tol = 2, 257, 1e-6
    z, _, _ = gaussian_shift_problem(V, N, 11)
    ls = np.log(np.full(V, 1.0 / V))
    trace = fit_priors(z, ls, max_iter=20, tol=0.0)["d_trace"]
    want = fit_priors(z, ls, max_iter=200, tol=tol)
    print(f"d trace {[f'{d:.3g}' for d in trace[:want['iterations'] + 1]]}, tol {tol}: {want['reason']} after {want['iterations']}")
    # no iterate's d lies within a factor 2 of tol, so rounding cannot move the decision
    assert all(d >= 2.0 * tol or d <= 0.5 * tol for d in trace[:want["iterations"]]) and want["reason"] == "tol" and want["iterations"] >= 2
    got = _fit(z, ls, max_iter=200, tol=tol)
    assert (got["reason"], got["iterations"], got["rows"]) == ("tol", want["iterations"], N)
    assert max(iterate_errors(got, want, N).values()) <= 1.0 and got["d"] <= tol
    # the cap: the same input, fewer iterations than it needs
    capped, want = _fit(z, ls, max_iter=want["iterations"] - 2, tol=tol), fit_priors(z, ls, max_iter=want["iterations"] - 2, tol=tol)
    assert (capped["reason"], capped["iterations"]) == ("cap", want["iterations"]) == (want["reason"], want["iterations"])
    assert max(iterate_errors(capped, want, N).values()) <= 1.0 and capped["d"] > tol


def test_edge_rows(cases):
    z, ls = (a.copy() for a in cases[(257, 65)])
    bad = z.copy()
    bad[3, 1], bad[200, 64], bad[256] = np.nan, np.inf, -np.inf
    want, got = fit_priors(bad, ls, max_iter=4, tol=0.0), _fit(bad, ls, max_iter=4, tol=0.0)
    assert (got["rows"], got["nan_rows"]) == (254, 3) == (want["rows"], want["nan_rows"])
    assert max(iterate_errors(got, want, 257).values()) <= 1.0 and np.isfinite(got["priors"]).all()
    # every row excluded
    none = _fit(np.full((5, 3), np.nan, dtype=np.float32), ls[:3].copy(), max_iter=4)
    assert (none["reason"], none["iterations"], none["rows"], none["nan_rows"], none["gain"], none["d"]) == ("empty", 0, 0, 5, 0.0, 0.0)
    assert np.abs(none["priors"] - np.exp(ls[:3])).max() <= 2.0 ** -52 and np.array_equal(none["priors"], none["mean_proba"]) and not none["log_ratio"].any()
    # a column of -inf (a class no row supports) and one the EM starves: prior 0 or tiny, the floor applies, nothing else breaks
    dead = z.copy()
    dead[:, 7] = -np.inf
    want, got = fit_priors(dead, ls, max_iter=8, tol=0.0), _fit(dead, ls, max_iter=8, tol=0.0)
    assert got["priors"][7] == 0.0 and got["mean_proba"][7] == 0.0 and want["log_ratio"][7] == np.log(FLOOR) - ls[7]
    assert abs(got["log_ratio"][7] - want["log_ratio"][7]) <= 2.0 ** -42           # (the device's log of 2^-1022 against numpy's)
    keep = np.arange(65) != 7
    for k in ("priors", "mean_proba", "log_ratio"):
        got[k], want[k] = got[k][keep], want[k][keep]
    assert np.isfinite(got["priors"]).all() and np.isfinite(got["log_ratio"]).all() and np.isfinite(got["gain"])
    assert max(iterate_errors(got, want, 257).values()) <= 1.0


def test_the_result_is_a_pure_function_of_the_arguments(cases):
    from slnlp import ops
    z, ls = cases[(1025, 202)]
    zd, lsd, state = _device(z, 205), torch.from_numpy(ls).cuda(), _state(0.5)
    out, scratch = torch.zeros(3 * 202 + 16, dtype=torch.float64, device="cuda"), torch.zeros(2 * 1025 + 202, dtype=torch.float64, device="cuda")
    first = ops.fit_priors(zd, lsd, state=state, max_iter=30, tol=1e-4, out=out, scratch=scratch).cpu().numpy().tobytes()
    assert ops.fit_priors(zd, lsd, state=state, max_iter=30, tol=1e-4, out=out, scratch=scratch).cpu().numpy().tobytes() == first   # over its own leftovers
    other = ops.fit_priors(zd, lsd, state=state, max_iter=30, tol=1e-4, out=torch.full((3 * 202 + 16,), float("nan"), dtype=torch.float64, device="cuda"),
                           scratch=torch.full((2 * 1025 + 202 + 64,), 7.0, dtype=torch.float64, device="cuda"))
    assert other.cpu().numpy().tobytes() == first
    assert ops.fit_priors(_device(z), lsd, state=state, max_iter=30, tol=1e-4).cpu().numpy().tobytes() == first       # another row stride


@pytest.mark.parametrize("N,V,ld,ld_out,beta", [(1, 1, None, None, None), (3, 2, None, None, 0.5), (257, 65, 68, 70, None), (1025, 202, None, 205, 0.5)])
def test_shift_logp(cases, N, V, ld, ld_out, beta):
    from slnlp import ops
    z, ls = cases[(N, V)]
    lw = np.random.RandomState(N).randn(V) - ls
    if V > 2:
        lw[V // 2] = -np.inf                                 # a class the target does not have
    zd, lwd, state = _device(z, ld), torch.from_numpy(lw).cuda(), _state(beta)
    out = torch.full((N, ld_out or V), float("nan"), dtype=torch.float32, device="cuda")[:, :V]
    assert ops.shift_logp(zd, lwd, state=state, out=out) is out
    got, want = out.cpu().numpy(), shift_logp(z, lw, beta or 1.0)
    err = ulp_error(got, want)
    print(f"[{N} x {V}, beta {beta}] max |device - fp64| = {err:.3f} float32 ulp; bits differ from the rounded reference in "
          f"{int((got != want.astype(np.float32)).sum())} of {got.size}")
    assert err <= 1.0
    if V > 2:
        assert (got[:, V // 2] == -np.inf).all()
    assert np.abs(np.exp(got.astype(np.float64)).sum(axis=1) - 1.0).max() <= V * 2.0 ** -23
    if V > 1:                                                # the arg-max, wherever one float32 step cannot decide it
        two = np.sort(want, axis=1)[:, -2:]
        clear = two[:, 1] - two[:, 0] > 2.0 * np.spacing(np.abs(two[:, 1]).astype(np.float32))
        assert clear.mean() >= 0.9 and np.array_equal(got.argmax(axis=1)[clear], want.argmax(axis=1)[clear])
    if ld_out:
        assert torch.isnan(out._base[:, V:]).all()           # the padding of out is not written
    # in place: the same bits
    same = zd.clone() if ld is None else _device(z, ld)
    assert ops.shift_logp(same, lwd, state=state, out=same) is same and same.cpu().numpy().tobytes() == ops.shift_logp(zd, lwd, state=state).cpu().numpy().tobytes()
    assert got.tobytes() == same.cpu().numpy().tobytes()


def test_shift_logp_rows_without_a_softmax(cases):
    from slnlp import ops
    z, ls = (a.copy() for a in cases[(257, 65)])
    z[3, 1], z[200, 64], z[256] = np.nan, np.inf, -np.inf
    lw = -ls
    got = ops.shift_logp(_device(z), torch.from_numpy(lw).cuda()).cpu().numpy()
    assert np.isnan(got[[3, 200, 256]]).all() and np.isfinite(np.delete(got, [3, 200, 256], axis=0)).all()
    assert ulp_error(got, shift_logp(z, lw)) <= 1.0
    none = ops.shift_logp(_device(z), torch.full((65,), float("-inf"), dtype=torch.float64, device="cuda")).cpu().numpy()
    assert np.isnan(none).all()                              # no class left


def test_invalid_arguments_leave_the_outputs_alone():
    from slnlp import _lib
    lib = _lib.load()
    N, V = 9, 5
    z = torch.zeros(N, V, dtype=torch.float32, device="cuda")
    ls = torch.full((V,), float(np.log(0.2)), dtype=torch.float64, device="cuda")
    table, state = (torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for n in (3 * V, 16))
    scratch = torch.full((2 * N + V,), 7.0, dtype=torch.float64, device="cuda")
    out = torch.full((N, V), 7.0, dtype=torch.float32, device="cuda")
    p = lambda t: t.data_ptr()

    def fit(**kw):
        a = dict(logp=p(z), ld=V, N=N, V=V, beta=None, ls=p(ls), max_iter=5, tol=1e-6, table=p(table), state=p(state), scratch=p(scratch),
                 bytes=8 * (2 * N + V))
        a.update(kw)
        rc = lib.slnlp_fit_priors(a["logp"], a["ld"], a["N"], a["V"], a["beta"], a["ls"], a["max_iter"], a["tol"], a["table"], a["state"],
                                  a["scratch"], a["bytes"], None)
        return rc, lib.slnlp_last_error().decode()
    for kw, text in (({"logp": None}, "null pointer"), ({"table": None}, "null pointer"), ({"N": 0}, "N=0 outside"), ({"V": 0}, "V=0 outside"),
                     ({"ld": V - 1}, "is less than V"), ({"max_iter": 1025}, "max_iter=1025"), ({"max_iter": -1}, "max_iter=-1"),
                     ({"tol": -1e-9}, "tol="), ({"tol": float("nan")}, "tol=nan"), ({"bytes": 8 * (2 * N + V) - 1}, "too small"),
                     ({"ls": p(ls) + 4}, "misaligned"), ({"table": p(z)}, "output table overlaps input logp"),
                     ({"state": p(table) + 8}, "outputs table and state overlap"), ({"scratch": p(ls)}, "output scratch overlaps input log_source")):
        rc, msg = fit(**kw)
        assert rc == 1 and "fit_priors" in msg and text in msg, (kw, rc, msg)

    def shift(**kw):
        a = dict(logp=p(z), ld=V, N=N, V=V, beta=None, lw=p(ls), out=p(out), ld_out=V)
        a.update(kw)
        rc = lib.slnlp_shift_logp(a["logp"], a["ld"], a["N"], a["V"], a["beta"], a["lw"], a["out"], a["ld_out"], None)
        return rc, lib.slnlp_last_error().decode()
    for kw, text in (({"lw": None}, "null pointer"), ({"out": None}, "null pointer"), ({"N": 2 ** 31}, "outside"), ({"ld_out": V - 1}, "ld_out=4 is less than V=5"),
                     ({"out": p(z) + 4}, "out overlaps logp without being logp itself"), ({"out": p(z), "ld": V + 1}, "out overlaps logp"),
                     ({"out": p(out) + 2}, "misaligned")):
        rc, msg = shift(**kw)
        assert rc == 1 and "shift_logp" in msg and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    for t in (table, state, scratch, out):
        assert (t == 7.0).all()
    assert not z.any()


# ------------------------------------------------------------------------------------------------------ estimator ----
GRU = dict(module="model.EncoderDecoderGRUAttn", module__embedding_size=24, module__hidden_size=32, module__num_layers=2)


def make_net(ds, seed, **kw):
    from slnlp.net import NeuralNetClassifier
    args = dict(module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y, module__batch_first=True, **GRU,
                criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1, optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05,
                max_epochs=2, batch_size=20, device="cuda", gradient_clipping={"gradient_clip_value": 0.5})
    args.update(kw)
    net = NeuralNetClassifier(**args)
    torch.manual_seed(seed)
    return net.initialize()


@pytest.fixture(scope="module")
def data():
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(140, seq_len=10, src_vocab=40, n_labels=5, seed=4, min_len=3)
    return ds[np.arange(100)], ds[np.arange(100, 140)]


@pytest.fixture(scope="module")
def fits(data):
    """Two two-epoch GRU fits, the first with a fitted temperature."""
    train, _ = data
    return [make_net(train, 21 + k, **({"calibration": {"method": "temperature"}} if k == 0 else {})).partial_fit(train) for k in range(2)]


def _raw(est, ds, calibrated=False):
    """The float32 log-probs ``predict_proba`` downloads, before the host softmax (a fit's: uncalibrated unless asked for)."""
    hidden = {} if calibrated else {k: est.__dict__.pop(k) for k in ("calibration_", "temperature_") if k in est.__dict__}
    own = "predict_nonlinearity" in est.__dict__              # (a fit's parameter; the wrappers' class attribute)
    keep = est.predict_nonlinearity
    est.predict_nonlinearity = "none"
    try:
        return est.predict_proba(ds)
    finally:
        if own:
            est.predict_nonlinearity = keep
        else:
            del est.predict_nonlinearity
        est.__dict__.update(hidden)


def test_prior_shift_on_a_fit(data, fits):
    import slnlp
    train, test = data
    net = fits[0]
    beta = net.calibration_["beta"]
    V, N = len(net.classes_), len(test)
    ps = slnlp.PriorShift(net, source=train)
    assert ps.fit(test, max_iter=5, tol=0.0) is ps
    z_train, z = _raw(net, train), _raw(net, test)
    source = fit_priors(z_train, np.zeros(V), beta=beta, max_iter=0, tol=0.0)["mean_proba"]
    assert np.abs(ps.source_priors_ - source / source.sum()).max() <= iterate_bound(1.0, len(train))
    want = fit_priors(z, np.log(ps.source_priors_), beta=beta, max_iter=5, tol=0.0)
    info = ps.prior_shift_
    print(f"source {ps.source_priors_}\npriors {ps.priors_}\ngain {info['gain']:.6g} after {info['iterations']} ({info['reason']}); error / bound "
          f"{iterate_errors(info, want, N)}")
    assert (info["reason"], info["iterations"], info["rows"], info["nan_rows"]) == ("cap", 6, N, 0)
    assert max(iterate_errors(info, want, N).values()) <= 1.0
    assert np.array_equal(ps.priors_, info["priors"]) and np.array_equal(ps.log_ratio_, info["log_ratio"])
    # predict_proba: the host softmax of the re-weighted device log-probs, which lie within one float32 ulp of the restatement
    raw = _raw(ps, test)
    assert raw.dtype == np.float32 and ulp_error(raw, shift_logp(z, ps.log_ratio_, beta)) <= 1.0
    proba = ps.predict_proba(test)
    assert proba.tobytes() == torch.softmax(torch.from_numpy(raw), dim=-1).numpy().tobytes()
    assert np.array_equal(ps.predict(test), ps.classes_[raw.argmax(axis=1)]) and ps.score(test) == float((raw.argmax(axis=1) == test.y).mean())
    # at T = 1 on request
    off = slnlp.PriorShift(net, source=ps.source_priors_, calibrated=False).fit(test, max_iter=5, tol=0.0)
    assert max(iterate_errors(off.prior_shift_, fit_priors(z, np.log(ps.source_priors_), max_iter=5, tol=0.0), N).values()) <= 1.0
    assert ulp_error(_raw(off, test), shift_logp(z, off.log_ratio_)) <= 1.0
    # the consumers of a fit's log-probs run on the wrapper, on the re-weighted log-probs
    rel = ps.reliability(test, bins=10)
    assert rel["rows"] == N and rel["temperature"] == 1.0 and abs(rel["accuracy"] - ps.score(test)) <= 1e-12
    labels, prob = ps.predict_topk(test, k=3)
    assert np.array_equal(labels[:, 0], ps.predict(test)) and np.abs(prob[:, 0] - proba.max(axis=1)).max() <= 1e-6
    assert ps.conformalize(train, alpha=0.2).predict_set(test)["sizes"].shape == (N,)
    # the default fit stops by itself or at the cap; known priors: the source's change no arg-max
    info = ps.fit(test).prior_shift_
    assert info["reason"] in ("tol", "cap") and 1 <= info["iterations"] <= 201 and info["gain"] >= -2.0 ** -40 and getattr(ps, "conformal_", None) is None
    ps.set_priors(ps.source_priors_)
    assert ps.prior_shift_ is None and np.abs(ps.log_ratio_).max() <= 2.0 ** -50       # (the priors are normalised once more: an ulp)
    assert np.array_equal(_raw(ps, test).argmax(axis=1), _raw(net, test, calibrated=True).argmax(axis=1))
    assert np.array_equal(ps.predict(test), net.predict(test))
    tilted = np.full(V, 1e-3)
    tilted[2] = 1.0
    assert (ps.set_priors(tilted).predict(test) == ps.classes_[2]).mean() >= (net.predict(test) == net.classes_[2]).mean()


def test_prior_shift_on_an_ensemble(data, fits):
    import slnlp
    train, test = data
    ens = slnlp.VotingEnsemble(fits)
    ps = slnlp.PriorShift(ens, source=train).fit(test, max_iter=5, tol=0.0)
    z = _raw(ens, test, calibrated=True)
    want = fit_priors(z, np.log(ps.source_priors_), max_iter=5, tol=0.0)
    assert max(iterate_errors(ps.prior_shift_, want, len(test)).values()) <= 1.0
    assert ulp_error(_raw(ps, test), shift_logp(z, ps.log_ratio_)) <= 1.0
    assert np.abs(ps.predict_proba(test).sum(axis=1) - 1.0).max() <= 1e-5 and ps.reliability(test)["rows"] == len(test)
    ps.set_priors(ps.source_priors_)
    assert np.array_equal(ps.predict(test), ens.predict(test))


# ------------------------------------------------------------------------------------------------------------ CLI ----
@pytest.mark.parametrize("source", ["train", "train_labels"])
def test_cli_writes_the_prior_shift_with_the_key(tmp_path, source):
    import csv
    import json
    import os

    import slnlp
    from slnlp import cli
    from slnlp.prior_shift import class_frequencies
    base = {"seed": 1, "cv": 2, "max_epochs": 2, "batch_size": 16, "test_size": 0.25, "scoring": ["neg_log_loss"],
            "model": "model.EncoderDecoderGRUAttn", "model_args": {"embedding_size": 16, "hidden_size": 32, "num_layers": 1, "dropout": 0.1},
            "optimizer_args": {"momentum": 0.9}, "gradient_clipping": {"gradient_clip_value": 0.5}, "grid_args": {"lr": [0.05]},
            "dataset_args": {"synthetic": {"n": 96, "seq_len": 10, "src_vocab": 40, "n_labels": 5, "seed": 4, "min_len": 3}}}
    if source == "train":
        with pytest.raises(ValueError, match="prior_shift: source='valid'"):      # before the grid search
            cli.run(cli.load_config(None, dict(base, workdir=str(tmp_path / "bad"), prior_shift={"source": "valid"})))
        assert not os.path.exists(tmp_path / "bad" / "grid_search_output.json")
    work = tmp_path / "run"
    gs, test_output = cli.run(cli.load_config(None, dict(base, workdir=str(work), prior_shift={"max_iter": 50, "tol": 1e-5, "source": source})))
    assert {"test_output.json", "test_prior_shift.json", "test_prior_shift_classes.csv"} <= set(os.listdir(work))
    got = json.load(open(work / "test_prior_shift.json"))
    assert set(got) == {"gain", "d", "reason", "iterations", "rows", "nan_rows", "source", "max_iter", "tol", "before", "after"}
    test_data, train_data = cli.load_dataset(base).split(0.25, 1)
    est = gs.best_estimator_
    V = len(est.classes_)
    assert (got["rows"], got["nan_rows"], got["source"], got["max_iter"], got["tol"]) == (len(test_data), 0, source, 50, 1e-5)
    assert got["reason"] in ("tol", "cap") and got["gain"] >= -2.0 ** -40
    assert set(got["before"]) == set(got["after"]) == {"accuracy", "balanced_accuracy", "log_loss"}
    assert got["before"]["accuracy"] == pytest.approx(test_output["test_accuracy"], abs=1e-12)
    assert got["before"]["log_loss"] == pytest.approx(-test_output["test_neg_log_loss"], abs=1e-12)
    # the same wrapper built by hand gives the file's numbers
    ps = slnlp.PriorShift(est, train_data if source == "train" else class_frequencies(train_data.y, V, 1.0)).fit(test_data, max_iter=50, tol=1e-5)
    assert (ps.prior_shift_["gain"], ps.prior_shift_["iterations"]) == (got["gain"], got["iterations"])
    assert got["after"]["accuracy"] == float((ps.predict(test_data) == test_data.y).mean())
    rows = list(csv.reader(open(work / "test_prior_shift_classes.csv")))
    assert rows[0] == ["class", "name", "source_prior", "estimated_prior", "test_frequency"] and len(rows) == V + 1
    assert [float(r[2]) for r in rows[1:]] == ps.source_priors_.tolist() and [float(r[3]) for r in rows[1:]] == ps.priors_.tolist()
    assert [float(r[4]) for r in rows[1:]] == (np.bincount(test_data.y, minlength=V) / len(test_data)).tolist()
