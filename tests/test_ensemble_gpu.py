"""GPU: voting ensembles on the device -- ``slnlp_ensemble_rows`` through ``ops.ensemble_rows`` and the C ABI against the numpy
restatement (tests/ensemble_ref.py, itself held to a direct fp64 computation on the CPU), ``VotingEnsemble`` and the CLI key.

The bounds: the three entropies of a row agree with the restatement to 1e-9 (absolute; relative above 1) -- the project's bound for
this fp64 arithmetic (``BOUND`` in tests/test_reliability_gpu.py); ``out`` lies within half a float32 spacing of the restatement's
fp64 value r plus 1e-9 max(1, |r|) -- one correct rounding plus the fp64 bound; -inf and NaN patterns are exactly equal; the
arg-max and ``n_disagree`` are compared on EVERY row (tests/test_ensemble_cpu.py shows the margin that allows it).

``test_ensemble_timing`` (no threshold: nothing on the parent commit does this job) measured on one MI355X, median of 12 calls at
N = 4000, V = 202, K = 5, soft voting: see profiles/ensemble_timing.json."""
import json
import os

import numpy as np
import pytest
import torch

from ensemble_ref import (FAMILIES, SHAPES, STRIDES, case_betas, case_weights, ensemble_ref, make_members, out_bound, spacing32,
                          uncertainty_ref)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPERATURE = {"method": "temperature"}
BOUND = 1e-9
NAN_ROW = [np.nan, np.nan, np.nan, -2.0]


def _padded(a, ld=None):
    """``a`` float32 [N, V] on the device, its rows ``ld`` floats apart (the padding is NaN: never to be read)."""
    N, V = a.shape
    buf = torch.full((N, ld or V), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(a).cuda()
    return buf[:, :V]


def _states(betas):
    from slnlp import ops
    return [None if b is None else ops.temperature_state(b, "cuda") for b in betas]


def _hold(tag, got_out, got_rows, want_out, want_rows, members):
    """One call against the restatement; returns (worst entropy difference, worst |out - r| as a share of its bound)."""
    assert got_out.dtype == np.float32 and got_out.shape == want_out.shape and got_rows.shape == want_rows.shape, tag
    bad = want_rows[:, 3] < 0
    assert np.isnan(got_out[bad]).all() and np.array_equal(got_rows[bad], want_rows[bad], equal_nan=True), tag
    g, r, gr, wr = got_out[~bad].astype(np.float64), want_out[~bad], got_rows[~bad], want_rows[~bad]
    assert not np.isnan(g).any() and np.array_equal(np.isinf(g), np.isinf(r)) and (g[np.isinf(g)] < 0).all(), tag     # the -inf pattern
    fin = np.isfinite(r)
    share = (np.abs(g[fin] - r[fin]) / out_bound(r[fin])).max(initial=0.0)
    assert share <= 1.0, (tag, share)
    d = np.abs(gr[:, :3] - wr[:, :3]) / np.maximum(1.0, np.abs(wr[:, :3]))
    assert np.isfinite(gr).all() and d.max(initial=0.0) <= BOUND, (tag, d.max(axis=0))
    # every row: the arg-max of the stored row and the members that disagree with it
    assert np.array_equal(np.argmax(got_out[~bad], axis=1), np.argmax(r, axis=1)), tag
    assert np.array_equal(gr[:, 3], wr[:, 3]), tag
    stored_top = np.argmax(got_out[~bad], axis=1)
    assert np.array_equal(gr[:, 3], sum((np.argmax(m[~bad], axis=1) != stored_top).astype(np.float64) for m in members)), tag
    return float(d.max(initial=0.0)), float(share)


# ------------------------------------------------------------------------------------------------- kernel, C ABI ----
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_V%d_K%d" % s)
def test_kernel_against_the_restatement(shape):
    from slnlp import ops
    N, V, K = shape
    lds, ld_out = STRIDES.get(shape, ((None,) * K, None))
    worst = [0.0, 0.0]
    for family in FAMILIES:
        members, _ = make_members(N, V, K, *family)
        dev = [_padded(m, ld) for m, ld in zip(members, lds)]
        for betas_on in (False, True):
            betas = case_betas(K, betas_on)
            states = _states(betas)
            for weights_on in (False, True):
                weights = case_weights(K, weights_on)
                for mode in ("soft", "log"):
                    tag = (shape, family, betas_on, weights_on, mode)
                    want_out, want_rows = ensemble_ref(members, betas, weights, mode)
                    buf = torch.full((N, ld_out or V), 7.0, dtype=torch.float32, device="cuda")
                    out, rows = ops.ensemble_rows(dev, states=states, weights=weights, voting=mode, out=buf[:, :V])
                    assert out.data_ptr() == buf.data_ptr() and rows.shape == (N, 4) and rows.dtype == torch.float64, tag
                    assert bool((buf[:, V:] == 7.0).all()), tag                     # the padding of out is not written
                    got_out, got_rows = out.cpu().numpy(), rows.cpu().numpy()
                    d, share = _hold(tag, got_out, got_rows, want_out, want_rows, members)
                    worst = [max(worst[0], d), max(worst[1], share)]
                    w = np.array(weights or [1.0] * K) / np.sum(weights or [1.0] * K)
                    assert got_rows[:, 2].min() >= -1e-12 and got_rows[:, 2].max() <= -(w * np.log(w)).sum() + 1e-12, tag
                    # without the diagnostics: the same out, bit for bit, and no rows
                    alone, none = ops.ensemble_rows(dev, states=states, weights=weights, voting=mode, diagnostics=False)
                    assert none is None and alone.cpu().numpy().tobytes() == got_out.tobytes(), tag
                    if V == 1:
                        assert np.abs(got_out).max() <= 1e-15 and np.abs(got_rows).max() <= 1e-15, tag
    print(f"{shape}: max entropy difference {worst[0]:.3e} (bound {BOUND}), max |out - r| / bound {worst[1]:.3f}")


def test_nan_and_minus_inf_entries():
    from slnlp import ops
    members, _ = make_members(33, 7, 3, 2.0, 0.6, 5)
    col = int(np.argmin(sum(m[6] for m in members)))
    nan, shared, single = ([m.copy() for m in members] for _ in range(3))
    nan[1][4, 2] = np.nan                                    # one NaN entry in one member's row
    for m in shared:                                         # one -inf column shared by all members
        m[6, col] = -np.inf
    single[2][6, col] = -np.inf                              # one -inf column in a single member
    split = [np.array([[0.0, -np.inf], [-1.0, -0.5]], dtype=np.float32), np.array([[-np.inf, 0.0], [-0.25, -2.0]], dtype=np.float32)]
    for name, ms in (("nan", nan), ("shared", shared), ("single", single), ("split", split)):
        dev = [_padded(m) for m in ms]
        for betas_on in (False, True):
            betas = case_betas(len(ms), betas_on)
            for mode in ("soft", "log"):
                want_out, want_rows = ensemble_ref(ms, betas, [1.0 + k for k in range(len(ms))], mode)
                out, rows = ops.ensemble_rows(dev, states=_states(betas), weights=[1.0 + k for k in range(len(ms))], voting=mode)
                got_out, got_rows = out.cpu().numpy(), rows.cpu().numpy()
                _hold((name, betas_on, mode), got_out, got_rows, want_out, want_rows, ms)
                if name == "nan":
                    assert np.isnan(got_out[4]).all() and np.array_equal(got_rows[4], NAN_ROW, equal_nan=True)
                    assert np.isfinite(np.delete(got_out, 4, axis=0)).all() and (np.delete(got_rows, 4, axis=0)[:, 3] >= 0).all()
                if name == "shared" or (name == "single" and mode == "log"):
                    assert got_out[6, col] == -np.inf and np.isfinite(np.delete(got_out[6], col)).all() and np.isfinite(got_rows).all()
                if name == "single" and mode == "soft":
                    assert np.isfinite(got_out).all() and np.isfinite(got_rows).all()
                if name == "split":                          # row 0: every class impossible for one member
                    assert np.isnan(got_out[0]).all() == (mode == "log") and (got_rows[0, 3] == -2.0) == (mode == "log")
                    assert np.isfinite(got_out[1]).all() and got_rows[1, 3] >= 0
                got = ops.ensemble_download((out, rows), per_row=True)
                assert {k: v for k, v in got.items() if k != "per_row"} == uncertainty_ref(got_rows)
                assert got["per_row"].tobytes() == got_rows.tobytes() and got["nan_rows"] == int((want_rows[:, 3] < 0).sum())


def test_the_result_is_a_pure_function_of_the_arguments():
    from slnlp import ops
    members, _ = make_members(300, 202, 4, 2.0, 0.6, 3)
    dev = [_padded(m) for m in members]
    states = _states(case_betas(4, True))
    for mode in ("soft", "log"):
        out, rows = ops.ensemble_rows(dev, states=states, weights=[1.0, 2.0, 3.0, 4.0], voting=mode)
        a = out.cpu().numpy().tobytes() + rows.cpu().numpy().tobytes()
        again = ops.ensemble_rows(dev, states=states, weights=[1.0, 2.0, 3.0, 4.0], voting=mode, out=torch.full_like(out, float("nan")))
        assert again[0].cpu().numpy().tobytes() + again[1].cpu().numpy().tobytes() == a
        # weights are normalised by the call: a common factor changes nothing ...
        scaled = ops.ensemble_rows(dev, states=states, weights=[2.0, 4.0, 6.0, 8.0], voting=mode)
        assert scaled[0].cpu().numpy().tobytes() + scaled[1].cpu().numpy().tobytes() == a
        # ... and beta = 1 from a state is beta = 1 as the null pointer
        ones = ops.ensemble_rows(dev, states=_states([1.0] * 4), voting=mode)
        null = ops.ensemble_rows(dev, voting=mode)
        assert ones[0].cpu().numpy().tobytes() == null[0].cpu().numpy().tobytes() != out.cpu().numpy().tobytes()
        assert ones[1].cpu().numpy().tobytes() == null[1].cpu().numpy().tobytes()


def test_one_member_is_scale_logp_and_a_member_listed_twice_is_itself():
    from slnlp import ops
    for family in FAMILIES:
        (m,), _ = make_members(257, 70, 1, *family)
        z = _padded(m, 72)
        for beta in (0.16, 1.0, 6.25):
            state = ops.temperature_state(beta, "cuda")
            want = ops.scale_logp(z, state).cpu().numpy()
            out, rows = ops.ensemble_rows([z], states=[state])
            got, r = out.cpu().numpy(), rows.cpu().numpy()
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= spacing32(want)).all(), (family, beta)      # one float32 ulp
            assert not r[:, 2].any() and not r[:, 3].any() and np.abs(r[:, 0] - r[:, 1]).max() <= 1e-12       # MI 0: l - mix is l - l
            for mode in ("soft", "log"):
                twice_out, twice_rows = ops.ensemble_rows([z, z], states=[state, state], weights=[1.0, 1.0], voting=mode)
                once_out, once_rows = ops.ensemble_rows([z], states=[state], voting=mode)
                a, b = twice_out.cpu().numpy().astype(np.float64), once_out.cpu().numpy().astype(np.float64)
                assert (np.abs(a - b) <= 2.0 * out_bound(b)).all(), (family, beta, mode)       # each within the bound of the same r
                d = np.abs(twice_rows.cpu().numpy() - once_rows.cpu().numpy())
                assert (d[:, :3] <= BOUND * np.maximum(1.0, np.abs(once_rows.cpu().numpy()[:, :3]))).all() and not d[:, 3].any(), (family, beta, mode)


def test_bad_arguments_return_codes_and_messages():
    import ctypes as C
    from slnlp import _lib, ops
    lib = _lib.load()
    members, _ = make_members(5, 3, 3, 2.0, 0.6, 1)
    dev = [_padded(m, ld) for m, ld in zip(members, (3, 4, 3))]
    states = [ops.temperature_state(0.5, "cuda"), None, ops.temperature_state(2.0, "cuda")]
    out = torch.full((5 * 3 + 16,), 7.0, dtype=torch.float32, device="cuda")
    rows = torch.full((5 * 4 + 16,), 9.0, dtype=torch.float64, device="cuda")
    p, st = _lib.ptr, _lib.stream_ptr()

    def call(**kw):
        a = dict(members=[p(z) for z in dev], ld=[3, 4, 3], betas=[p(s) for s in states], weights=[1.0, 2.0, 3.0], K=3, N=5, V=3, mode=0,
                 out=p(out), ld_out=3, rows=p(rows))
        a.update(kw)
        arr = lambda t, v: None if v is None else (t * len(v))(*v)
        rc = lib.slnlp_ensemble_rows(arr(C.c_void_p, a["members"]), arr(C.c_int64, a["ld"]), arr(C.c_void_p, a["betas"]),
                                     arr(C.c_double, a["weights"]), a["K"], a["N"], a["V"], a["mode"], a["out"], a["ld_out"], a["rows"], st)
        return rc, lib.slnlp_last_error().decode()
    m = [p(z) for z in dev]
    for kw, text in (({"members": None}, "null pointer"), ({"ld": None}, "null pointer"), ({"out": None}, "null pointer"),
                     ({"members": [m[0], None, m[2]]}, "member 1 is a null pointer"), ({"K": 0}, "K=0 outside 1..32"), ({"K": 33}, "K=33 outside 1..32"),
                     ({"N": 0}, "N=0 outside"), ({"N": 2 ** 31}, "N=2147483648 outside"), ({"V": 0}, "V=0 outside"), ({"V": 2 ** 31}, "V=2147483648"),
                     ({"mode": 2}, "mode=2"), ({"ld": [3, 2, 3]}, "ld[1]=2 is less than V=3"), ({"ld_out": 2}, "ld_out=2 is less than V=3"),
                     ({"weights": [1.0, 0.0, 1.0]}, "weights[1]=0"), ({"weights": [1.0, 1.0, float("nan")]}, "weights[2]=nan"),
                     ({"weights": [float("inf"), 1.0, 1.0]}, "weights[0]=inf"), ({"members": [m[0] + 2, m[1], m[2]]}, "member 0 is not 4-byte aligned"),
                     ({"out": p(out) + 2}, "out is not 4-byte aligned"), ({"betas": [p(states[0]) + 4, None, None]}, "beta of member 0 is not 8-byte"),
                     ({"rows": p(rows) + 16}, "rows is not 32-byte aligned"), ({"out": m[1] + 4 * 18}, "out overlaps member 1"),
                     ({"out": m[0]}, "out overlaps member 0"), ({"rows": p(states[2]) // 32 * 32}, "rows overlaps the beta of member 2"),
                     ({"out": p(states[0])}, "out overlaps the beta of member 0"), ({"rows": p(out) // 32 * 32 + 32}, "out and rows overlap")):
        rc, msg = call(**kw)
        assert rc == 1 and "ensemble_rows" in msg and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()                                                    # no sticky error: nothing faulted ...
    assert bool((out == 7.0).all()) and bool((rows == 9.0).all())               # ... and nothing was launched
    # the nullable ones: betas, an entry of them, weights, rows
    assert call(betas=None, weights=None, rows=None)[0] == 0
    torch.cuda.synchronize()
    assert bool((out[:15] != 7.0).all()) and bool((out[15:] == 7.0).all()) and bool((rows == 9.0).all())
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert bool((rows[:20] != 9.0).all()) and bool((rows[20:] == 9.0).all())
    want = ensemble_ref(members, [0.5, None, 2.0], [1.0, 2.0, 3.0])
    _hold("abi", out[:15].view(5, 3).cpu().numpy(), rows[:20].view(5, 4).cpu().numpy(), *want, members)
    assert lib.slnlp_abi_version() == 1
    # the front-end's own checks
    for kw in ({"voting": "hard"}, {"weights": [1.0, 2.0]}, {"weights": [1.0, 0.0, 1.0]}, {"states": states[:2]}, {"states": [out, None, None]},
               {"out": torch.empty(5, 4, device="cuda")}):
        with pytest.raises(ValueError, match="ensemble_rows"):
            ops.ensemble_rows(dev, **kw)
    for bad in ([], dev * 11, [dev[0], dev[1][:4]], [dev[0], dev[1].double()], [dev[0], dev[1].cpu()], dev[0]):
        with pytest.raises(ValueError, match="ensemble_rows"):
            ops.ensemble_rows(bad)
    with pytest.raises(ValueError, match="no diagnostics"):
        ops.ensemble_download(ops.ensemble_rows(dev, diagnostics=False))


def test_ensemble_timing():
    """No threshold: one call at N = 4000, V = 202, K = 5 with and without the diagnostics, median of 12 event-timed calls after
    a warm-up call each, written to profiles/ensemble_timing.json."""
    from slnlp import ops
    members, _ = make_members(4000, 202, 5, 2.0, 0.6, 1)
    dev = [_padded(m) for m in members]
    out = torch.empty(4000, 202, dtype=torch.float32, device="cuda")
    res = {}
    for mode in ("soft", "log"):
        for diagnostics in (True, False):
            ops.ensemble_rows(dev, voting=mode, diagnostics=diagnostics, out=out)
            times = []
            for _ in range(12):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                ops.ensemble_rows(dev, voting=mode, diagnostics=diagnostics, out=out)
                t1.record()
                t1.synchronize()
                times.append(t0.elapsed_time(t1) * 1e3)
            res[f"{mode}_{'with' if diagnostics else 'without'}_diagnostics_us"] = float(np.median(times))
    print(res)
    assert all(np.isfinite(v) and v > 0.0 for v in res.values())
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ensemble_timing.json"), "w") as f:
        json.dump({"test": "tests/test_ensemble_gpu.py::test_ensemble_timing", "device": torch.cuda.get_device_name(0), "N": 4000, "V": 202, "K": 5,
                   "calls": 12, "statistic": "median", **res}, f, indent=1)
        f.write("\n")


# ------------------------------------------------------------------------------------------------------ estimator ----
from test_calibration_gpu import make_net, raw_logp  # noqa: E402


@pytest.fixture(scope="module")
def ds():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(120, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


@pytest.fixture(scope="module")
def fits(ds):
    """Three tiny Transformer fits, two epochs each, the second with a fitted temperature."""
    return [make_net(ds, seed=11 + k, max_epochs=2, **({"calibration": TEMPERATURE} if k == 1 else {})).partial_fit(ds) for k in range(3)]


def _noisy_labels(data, V):
    rs = np.random.RandomState(0)
    y = np.asarray(data.y, dtype=np.int64)
    return np.where(rs.rand(len(y)) < 0.3, rs.randint(0, V, size=len(y)), y)


def _raw_out(ens, data):
    """The ensemble's float32 log-probs as ``predict_proba`` downloads them, before the host softmax."""
    ens.predict_nonlinearity = "none"
    try:
        return ens.predict_proba(data)
    finally:
        del ens.predict_nonlinearity


@pytest.mark.parametrize("voting,weights", [("soft", None), ("log", [1.0, 2.0, 3.0])])
def test_voting_ensemble_against_the_restatements(ds, fits, voting, weights):
    from bootstrap_ref import bootstrap_ref
    from confusion_ref import class_report_ref, confusion_ref, pairs_ref, topk_ref
    from reliability_ref import reliability_ref, rows_ref
    from slnlp import metrics
    from slnlp.ensemble import VotingEnsemble
    assert fits[1].temperature_ != 1.0 and getattr(fits[0], "calibration_", None) is None
    ens = VotingEnsemble(fits, voting=voting, weights=weights)
    members = [raw_logp(m, ds) for m in fits]
    betas = [None, fits[1].calibration_["beta"], None]
    want_out, want_rows = ensemble_ref(members, betas, weights, voting)
    # predict_proba: the host softmax of the device's log-probs, which lie within the out bound of the restatement
    z = _raw_out(ens, ds)
    assert z.dtype == np.float32 and (np.abs(z.astype(np.float64) - want_out) <= out_bound(want_out)).all()
    proba = ens.predict_proba(ds)
    assert proba.tobytes() == torch.softmax(torch.from_numpy(z), dim=-1).numpy().tobytes()
    assert np.abs(proba - np.exp(want_out)).max() <= 1e-6 and np.array_equal(ens.predict(ds), ens.classes_[np.argmax(z, axis=1)])
    assert ens.score(ds) == float((np.argmax(z, axis=1) == ds.y).mean())
    off, want_off = _raw_out(VotingEnsemble(fits, voting=voting, weights=weights, calibrated=False), ds), ensemble_ref(members, None, weights, voting)[0]
    assert (np.abs(off.astype(np.float64) - want_off) <= out_bound(want_off)).all() and not np.array_equal(off, z)
    # uncertainty
    unc = ens.uncertainty(ds, per_row=True)
    rows = unc.pop("per_row")
    assert unc == uncertainty_ref(rows) and unc["rows"] == len(ds) and unc["nan_rows"] == 0
    assert (np.abs(rows[:, :3] - want_rows[:, :3]) <= BOUND * np.maximum(1.0, np.abs(want_rows[:, :3]))).all()
    assert np.array_equal(rows[:, 3], sum((np.argmax(m, axis=1) != np.argmax(z, axis=1)).astype(np.float64) for m in members))
    assert rows[:, 2].min() >= -1e-12 and rows[:, 2].max() <= np.log(3.0) and "per_row" not in ens.uncertainty(ds)
    # the consumers of one fit's log-probs, fed the ensemble's: their own restatements on the downloaded log-probs
    y = _noisy_labels(ds, len(ens.classes_))
    rel = ens.reliability(ds, y=y, bins=10)
    t = rows_ref(z, y, 10)[:, 0] * 10
    assert not np.any((np.abs(t - np.round(t)) <= 1e-6) & (np.round(t) > 0) & (np.round(t) < 10))      # no row near an inner bin edge
    ref = reliability_ref(z, y, 10)
    assert rel["temperature"] == 1.0 and (rel["rows"], rel["bad_labels"], rel["nan_rows"]) == (len(ds), 0, 0)
    for k in ("ece", "mce", "brier", "nll", "accuracy", "confidence"):
        assert abs(rel[k] - ref[k]) <= BOUND * max(1.0, abs(ref[k])), (k, rel[k], ref[k])
    ea = ens.error_analysis(ds, y=y, pairs=5, top_k=3)
    V = len(ens.classes_)
    pred = np.argmax(z, axis=1)
    counts = confusion_ref(pred, y, V)
    assert np.array_equal(ea["confusion"], counts[:V * V].reshape(V, V)) and ea["accuracy"] == float((pred == y).mean())
    assert ea["pairs"] == [(int(t_), int(p_), int(c)) for t_, p_, c in pairs_ref(counts, V, 5) if c > 0]
    report, macro = class_report_ref(np.bincount(y, minlength=V), np.bincount(pred, minlength=V), np.bincount(y[pred == y], minlength=V))
    assert all(np.abs(ea["report"][k] - report[k]).max() <= 1e-12 for k in ("precision", "recall", "f1")) and ea["macro"] == pytest.approx(macro, abs=1e-12)
    idx, prob = topk_ref(z, 3)
    assert np.array_equal(ea["topk"][0], ens.classes_[idx]) and np.abs(ea["topk"][1] - prob).max() <= BOUND
    labels, top = ens.predict_topk(ds, k=3)
    assert np.array_equal(labels, ea["topk"][0]) and top.tobytes() == ea["topk"][1].tobytes()
    res = ens.score_interval(ds, y=y, replicates=200, seed=3, return_replicates=True)
    p_, picked, rank, cnt = metrics.reduce_rows(torch.from_numpy(z), torch.from_numpy(y))
    point = metrics.scores_from_rows(list(metrics.BOOT_COLUMNS), y, p_, picked, rank, cnt, V)
    boot = bootstrap_ref(y, p_, rank, rows_ref(z, y, 15)[:, :3], V, 2, 200, 3)[0]
    reps = res["replicate_scores"]
    assert res["names"] == [*metrics.BOOT_COLUMNS, "confidence", "neg_brier", "neg_log_loss"] and all(res[n]["point"] == point[n] for n in point)
    assert reps[:, 0].tobytes() == boot[:, 0].tobytes() and reps[:, 8].tobytes() == boot[:, 8].tobytes()
    assert np.abs(reps[:, 1:8] - boot[:, 1:8]).max() <= BOUND
    signed = boot[:, 9:] * np.array([1.0, -1.0, -1.0])
    assert (np.abs(reps[:, 9:] - signed) <= BOUND * np.maximum(1.0, np.abs(signed))).all()
    # is the ensemble really better: the paired bootstrap in both orders, against a net and against an ensemble
    for other in (fits[0], VotingEnsemble(fits[:1])):
        ab = other.compare(ens, ds, y=y, replicates=100, seed=2, return_replicates=True)
        ba = ens.compare(other, ds, y=y, replicates=100, seed=2, return_replicates=True)
        assert np.array_equal(ab["replicate_scores"], -ba["replicate_scores"]) and ab["names"] == ba["names"] and ab["rows"] == len(ds)
        for n in ab["names"]:
            assert ab[n]["point"] == -ba[n]["point"] and ab[n]["mean"] == -ba[n]["mean"] and ab[n]["std"] == ba[n]["std"], n
            assert abs(ab[n]["lower"] + ba[n]["upper"]) <= 1e-12 and abs(ab[n]["upper"] + ba[n]["lower"]) <= 1e-12, n
    with pytest.raises(ValueError, match=f"score_interval: 1 of 120 labels lie outside the {V} classes of the log-probs"):
        ens.score_interval(ds, y=np.where(np.arange(120) == 3, V, y), replicates=5)


def test_a_single_member_ensemble_and_member_scores(ds, fits):
    from slnlp.ensemble import VotingEnsemble
    from slnlp.net import ScoringWrapper
    for k, net in enumerate(fits):
        one = VotingEnsemble([net])
        unc = one.uncertainty(ds, per_row=True)
        assert unc["mutual_information"] == 0.0 and unc["disagreement_rate"] == 0.0 and unc["mean_disagreement"] == 0.0
        assert not unc["per_row"][:, 2:].any() and np.abs(unc["per_row"][:, 0] - unc["per_row"][:, 1]).max() <= 1e-12
        assert np.array_equal(one.predict(ds), net.predict(ds)) and np.abs(one.predict_proba(ds) - net.predict_proba(ds)).max() <= 1e-6
    names = ["accuracy", "neg_log_loss", "f1_macro", "top3_accuracy", "neg_brier"]
    ens = VotingEnsemble(fits)
    got = ens.member_scores(ds, names)
    labels = np.arange(len(ens.classes_))
    assert set(got) == {"ensemble", "members"} and len(got["members"]) == 3
    for est, scores in ((ens, got["ensemble"]), *zip(fits, got["members"])):
        assert scores == {n: float(ScoringWrapper(n, labels)(est, ds, ds.y)) for n in names}
    assert ens.member_scores(ds, "accuracy")["ensemble"] == {"accuracy": ens.score(ds)}


# ------------------------------------------------------------------------------------------------------------ CLI ----
def test_cli_writes_the_ensemble_with_the_key(tmp_path):
    from slnlp import cli
    from slnlp.ensemble import VotingEnsemble
    from slnlp.net import NeuralNetClassifier
    base = {"seed": 1, "cv": 2, "max_epochs": 2, "batch_size": 16, "test_size": 0.25, "scoring": ["neg_log_loss", "f1_macro"],
            "model": "model.Transformer", "model_args": {"embedding_size": 16, "hidden_size": 32, "num_layers": 1, "dropout": 0.1, "num_heads": 2},
            "optimizer_args": {"momentum": 0.9}, "gradient_clipping": {"gradient_clip_value": 0.5}, "grid_args": {"lr": [0.05]},
            "dataset_args": {"synthetic": {"n": 96, "seq_len": 10, "src_vocab": 40, "n_labels": 5, "seed": 4, "min_len": 3}}}
    with pytest.raises(ValueError, match="ensemble: members=1"):                # before the grid search
        cli.run(cli.load_config(None, dict(base, workdir=str(tmp_path / "bad"), ensemble={"members": 1})))
    assert not os.path.exists(tmp_path / "bad" / "grid_search_output.json")
    work = tmp_path / "run"
    gs, test_output = cli.run(cli.load_config(None, dict(base, workdir=str(work), ensemble={"members": 3, "voting": "log"},
                                                         confidence_intervals={"replicates": 50, "seed": 5})))
    assert {"test_output.json", "test_ensemble.json", "ensemble", "final", "params.pt"} <= set(os.listdir(work))
    assert sorted(os.listdir(work / "ensemble")) == ["member1", "member2"] and "params.pt" in os.listdir(work / "ensemble" / "member1")
    got = json.load(open(work / "test_ensemble.json"))
    assert set(got) == {"members", "voting", "scores", "uncertainty", "single_vs_ensemble"} and (got["members"], got["voting"]) == (3, "log")
    names = ["test_accuracy", "test_neg_log_loss", "test_f1_macro"]
    assert sorted(got["scores"]["ensemble"]) == sorted(names) and len(got["scores"]["members"]) == 3
    assert got["scores"]["members"][0] == pytest.approx(test_output, abs=1e-12)          # member 0 is the refit
    # the members read back from the files give the ensemble the file describes
    dataset = cli.load_dataset(base)
    test_data, _ = dataset.split(0.25, 1)
    members = [gs.best_estimator_]
    for i in (1, 2):
        net = NeuralNetClassifier(**cli.build_net_params(dict(base, workdir=None), dataset, "cuda:0")).set_params(**gs.best_params_).initialize()
        net.load_params(str(work / "ensemble" / f"member{i}"))
        net.classes_ = gs.best_estimator_.classes_
        members.append(net)
    ens = VotingEnsemble(members, voting="log")
    again = ens.member_scores(test_data, ["accuracy", "neg_log_loss", "f1_macro"])
    assert {f"test_{n}": v for n, v in again["ensemble"].items()} == got["scores"]["ensemble"]
    assert got["uncertainty"] == ens.uncertainty(test_data) and got["uncertainty"]["rows"] == len(test_data)
    cmp_ = got["single_vs_ensemble"]
    assert (cmp_["replicates"], cmp_["level"], cmp_["seed"], cmp_["rows"]) == (50, 0.95, 5, len(test_data))
    want = gs.best_estimator_.compare(ens, test_data, replicates=50, seed=5)
    assert cmp_["accuracy"] == want["accuracy"] and cmp_["neg_log_loss"] == want["neg_log_loss"]
