"""CPU: the host side of the label-shift adaptation -- the numpy restatement the GPU tests lean on (tests/prior_shift_ref.py): EM's
monotone likelihood, its fixed point, the ``max_iter = 0`` mean prediction, the recovery of a shifted prior on Gaussian data --
then ``PriorShift``'s argument checks, the CLI key, and the C ABI's argument checks (the library loads without a GPU)."""
import os
import re

import numpy as np
import pytest

from prior_shift_ref import FLOOR, counted_rows, fit_priors, gaussian_shift_problem, shift_logp, ulp_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECOVERY = [(2, 257, 11), (5, 2000, 12)]                     # (V, N, seed)


def softmax64(z, beta=1.0):
    a = np.float64(beta) * np.asarray(z, dtype=np.float64)
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.fixture(scope="module")
def problems():
    return {(V, N): gaussian_shift_problem(V, N, seed) for V, N, seed in RECOVERY}


def test_the_gain_never_goes_down(problems):
    for (V, N), (z, _, _) in problems.items():
        for beta in (1.0, 0.5):
            r = fit_priors(z, np.log(np.full(V, 1.0 / V)), beta=beta, max_iter=50, tol=0.0)
            steps = np.diff(r["gain_trace"])
            print(f"[{V} x {N}, beta {beta}] gain {r['gain_trace'][0]:.6g} -> {r['gain']:.6g}, smallest step {steps.min():.3g}")
            # (tol = 0 still stops a run whose priors stop moving in fp64 altogether: d = 0)
            assert (r["reason"] == "cap" and r["iterations"] == 51 or r["reason"] == "tol" and r["d"] == 0.0) and len(r["gain_trace"]) == r["iterations"] > 3
            assert steps.min() >= -2.0 ** -40 and r["gain_trace"][0] >= -2.0 ** -40


def test_the_result_is_a_fixed_point_to_tol(problems):
    """The EM map is a contraction near its fixed point, so the step after the one that stopped the iteration is no larger."""
    for (V, N), (z, _, _) in problems.items():
        ls = np.log(np.full(V, 1.0 / V))
        for tol in (1e-6, 1e-10):
            r = fit_priors(z, ls, max_iter=200, tol=tol)
            assert r["reason"] == "tol" and r["d"] <= tol and r["d_trace"][-1] == r["d"] and len(r["d_trace"]) == r["iterations"]
            assert all(d > tol for d in r["d_trace"][:-1])
            again = softmax64(z.astype(np.float64) + r["log_ratio"]).mean(axis=0)
            assert np.abs(again - r["priors"]).max() <= tol
            assert abs(r["priors"].sum() - 1.0) <= 1e-12
            assert np.array_equal(r["log_ratio"], np.log(np.maximum(r["priors"], FLOOR)) - ls)


def test_max_iter_zero_is_the_mean_prediction(problems):
    for (V, N), (z, _, _) in problems.items():
        for beta in (1.0, 0.5):
            r = fit_priors(z, np.log(np.full(V, 1.0 / V)), beta=beta, max_iter=0, tol=0.0)
            want = softmax64(z, beta).mean(axis=0)
            assert r["reason"] == "cap" and r["iterations"] == 1 and r["rows"] == N and r["nan_rows"] == 0
            assert np.array_equal(r["priors"], r["mean_proba"]) and np.abs(r["priors"] - want).max() <= 1e-15
    # with the source prior at the mean prediction the first step changes nothing: d = 0 <= tol at once
    z = problems[(5, 2000)][0]
    r = fit_priors(z, np.log(softmax64(z).mean(axis=0)), max_iter=5, tol=1e-15)
    assert r["reason"] == "tol" and r["iterations"] == 1 and r["d"] <= 1e-15


def test_recovery_of_the_target_prior(problems):
    """Exact source posteriors under a uniform prior, rows drawn under a Dirichlet(0.5) prior: the estimate's L1 distance to the
    sample's class frequencies is at most 0.1 times the source prior's."""
    for (V, N), (z, y, pi_t) in problems.items():
        # the draw itself: rows are normalised posteriors, and the labels follow the target prior (a frequency's standard
        # deviation is at most 1 / (2 sqrt N): five of them per class)
        assert z.dtype == np.float32 and z.shape == (N, V) and np.abs(np.exp(z.astype(np.float64)).sum(axis=1) - 1.0).max() <= V * 2.0 ** -22
        freq = np.bincount(y, minlength=V) / N
        assert np.abs(freq - pi_t).max() <= 2.5 / np.sqrt(N)
        source = np.full(V, 1.0 / V)
        r = fit_priors(z, np.log(source), max_iter=200, tol=1e-6)
        est, base = np.abs(r["priors"] - freq).sum(), np.abs(source - freq).sum()
        print(f"[{V} x {N}] L1(estimate, frequencies) = {est:.4g}, L1(source, frequencies) = {base:.4g}, ratio {est / base:.4g}; "
              f"{r['reason']} after {r['iterations']}")
        assert r["reason"] == "tol"
        assert est <= 0.1 * base


def test_excluded_rows_and_the_empty_set():
    z, _, _ = gaussian_shift_problem(3, 40, 5)
    ls = np.log(np.array([0.2, 0.3, 0.5]))
    bad = z.copy()
    bad[3, 1], bad[7, 0], bad[9] = np.nan, np.inf, -np.inf
    assert np.array_equal(np.flatnonzero(~counted_rows(bad)), [3, 7, 9])
    got, want = fit_priors(bad, ls, max_iter=8, tol=0.0), fit_priors(np.delete(z, [3, 7, 9], axis=0), ls, max_iter=8, tol=0.0)
    assert got["rows"] == 37 and got["nan_rows"] == 3
    assert np.array_equal(got["priors"], want["priors"]) and got["gain"] == want["gain"]
    none = fit_priors(np.full((4, 3), np.nan, dtype=np.float32), ls)
    assert none["reason"] == "empty" and none["iterations"] == 0 and none["rows"] == 0 and none["nan_rows"] == 4 and none["gain"] == 0.0
    assert np.array_equal(none["priors"], np.exp(ls)) and not none["log_ratio"].any()
    # a class without any support: its prior underflows towards 0, the floor keeps the log-ratio finite
    dead = z.copy()
    dead[:, 2] = -np.inf
    r = fit_priors(dead, ls, max_iter=8, tol=0.0)
    assert r["priors"][2] == 0.0 and r["log_ratio"][2] == np.log(FLOOR) - ls[2] and np.isfinite(r["log_ratio"]).all()
    assert np.isfinite(r["priors"]).all() and abs(r["priors"].sum() - 1.0) <= 1e-12 and np.isfinite(r["gain"])


def normalised_rows(N, V, seed):
    """Float32 log-probs normalised as well as float32 allows: columns 0 .. V-2 are the float32 log-probs of a random softmax,
    the last column is the float32 nearest to ln(1 - the others' mass), so ONE rounding separates the row from sum exp = 1."""
    rng = np.random.RandomState(seed)
    logits = 2.0 * rng.randn(N, V)
    logits[:, -1] = logits.max(axis=1) + 0.5                 # the closing column holds the largest mass: the others stay below 1 / 2
    p = softmax64(logits)
    z = np.log(p).astype(np.float32)
    z[:, -1] = np.log1p(-np.exp(z[:, :-1].astype(np.float64)).sum(axis=1)).astype(np.float32)
    return z


def test_a_zero_shift_reproduces_a_normalised_input():
    """log_w = 0, beta = 1.  For the rows above the logsumexp of the float32 row is r = p_last z_last delta with |delta| <= 2^-24
    (the closing column's one rounding; fp64 noise of 1e-16 beside it).  |r| < 2^-24 |z_last| < spacing(z_last), and for every
    other column |r| <= 2^-24 / e < 2^-24 ln 2 <= 2^-24 |z_c| < spacing(z_c) because p_c < 1 / 2: z - r lies within one float32
    step of z, and rounding to nearest cannot leave that step."""
    for N, V, seed in ((64, 2, 1), (64, 7, 2), (16, 202, 3)):
        z = normalised_rows(N, V, seed)
        assert (z[:, :-1] < np.log(0.5)).all() and (np.abs(z[:, -1]) >= 1e-3).all() and (z < 0).all()
        out = shift_logp(z, np.zeros(V)).astype(np.float32)
        err = np.abs(out.astype(np.float64) - z.astype(np.float64)) / np.spacing(np.abs(z)).astype(np.float64)
        print(f"[{N} x {V}] max |shift(z) - z| = {err.max():.3f} float32 ulp; {int((out != z).sum())} of {z.size} values moved")
        assert err.max() <= 1.0
        assert np.array_equal(out.argmax(axis=1), z.argmax(axis=1))
    one = shift_logp(np.array([[0.0], [-3.0]], dtype=np.float32), np.zeros(1))
    assert np.array_equal(one, np.zeros((2, 1)))             # V = 1: the only class has probability 1


def test_shift_rules():
    z, _, _ = gaussian_shift_problem(4, 9, 6)
    lw = np.array([0.3, -np.inf, -1.0, 0.0])
    out = shift_logp(z, lw, beta=0.5)
    assert (out[:, 1] == -np.inf).all() and np.isfinite(np.delete(out, 1, axis=1)).all()
    assert np.abs(np.exp(out).sum(axis=1) - 1.0).max() <= 1e-12
    want = softmax64(z, 0.5) * np.exp(lw)
    assert np.abs(np.exp(out) - want / want.sum(axis=1, keepdims=True)).max() <= 1e-12
    bad = z.copy()
    bad[2, 0], bad[5] = np.nan, np.inf
    out = shift_logp(bad, np.zeros(4))
    assert np.isnan(out[[2, 5]]).all() and np.isfinite(np.delete(out, [2, 5], axis=0)).all()
    assert np.isnan(shift_logp(z, np.full(4, -np.inf))).all()            # no class left
    assert ulp_error(np.float32([1.0, np.nan, -np.inf]), np.float64([1.0, np.nan, -np.inf])) == 0.0
    assert ulp_error(np.float32([1.0]), np.float64([1.0 + 2.0 ** -23])) == 1.0 and ulp_error(np.float32([np.nan]), np.float64([1.0])) == np.inf


def test_estimator_surface_without_a_gpu():
    import slnlp
    from slnlp.data import synthetic_dataset
    from slnlp.net import NeuralNetClassifier
    from slnlp.prior_shift import PriorShift, class_frequencies, normalised_priors
    assert slnlp.PriorShift is PriorShift and "PriorShift" in slnlp.__all__
    for name in ("predict_proba", "predict", "score", "predict_topk", "reliability", "ranking", "error_analysis", "score_interval", "compare",
                 "conformalize", "predict_set", "coverage"):
        assert getattr(PriorShift, name) is getattr(NeuralNetClassifier, name), name

    def fitted(n_classes, device="cuda:0"):
        net = NeuralNetClassifier(module="model.Transformer", device=device)
        net.initialized_, net.classes_ = True, np.arange(n_classes)
        return net
    base = fitted(4)
    with pytest.raises(RuntimeError, match="PriorShift: the base must be initialized"):
        PriorShift(NeuralNetClassifier(module="model.Transformer"), [0.25] * 4)
    with pytest.raises(ValueError, match="base must be a NeuralNetClassifier or a VotingEnsemble"):
        PriorShift("net", [0.25] * 4)
    with pytest.raises(ValueError, match=r"classes \[1, 3\] have prior 0"):
        PriorShift(base, [0.5, 0.0, 0.5, 0.0])
    for wrong in ([0.5, 0.5], np.full((2, 2), 0.25), 0.25, None, "abcd"):
        with pytest.raises(ValueError, match="expected 4 probabilities or counts"):
            PriorShift(base, wrong)
    for bad in ([0.5, -0.1, 0.3, 0.3], [0.5, float("nan"), 0.2, 0.3], [1.0, float("inf"), 1.0, 1.0]):
        with pytest.raises(ValueError, match="must be finite and >= 0"):
            PriorShift(base, bad)
    for smoothing in (-1.0, float("inf"), "1", True):
        with pytest.raises(ValueError, match="smoothing="):
            PriorShift(base, [0.25] * 4, smoothing=smoothing)
    ps = PriorShift(base, [3, 0, 1, 0], smoothing=1.0, calibrated=False)            # counts: smoothing fills the empty classes
    assert ps.calibration_ is None and ps.temperature_ == 1.0 and ps.initialized_ and np.array_equal(ps.classes_, np.arange(4))
    assert ps.get_params(deep=False) == {"base": base, "source": [3, 0, 1, 0], "calibrated": False, "smoothing": 1.0}
    assert np.array_equal(ps._source_priors(), np.array([4.0, 1.0, 2.0, 1.0]) / 8.0)
    assert np.array_equal(class_frequencies(np.array([0, 0, 2, 0]), 4, 1.0), ps._source_priors())
    assert np.array_equal(normalised_priors("x", [1, 1, 2], 3), [0.25, 0.25, 0.5])
    with pytest.raises(ValueError, match=r"classes \[1, 3\] have prior 0"):
        class_frequencies(np.array([0, 0, 2, 0]), 4)
    with pytest.raises(ValueError, match="1 of 3 labels lie outside the 2 classes"):
        class_frequencies(np.array([0, 1, 2]), 2)
    # before fit / set_priors everything that needs log-probs refuses, before any forward pass
    ds = synthetic_dataset(6, seq_len=8, src_vocab=20, n_labels=4, seed=1, min_len=3)
    for call in (lambda: ps.predict_proba(ds), lambda: ps.predict(ds), lambda: ps.reliability(ds), lambda: ps.predict_topk(ds, k=2),
                 lambda: ps.ranking(ds)):
        with pytest.raises(RuntimeError, match="PriorShift: no target priors yet"):
            call()
    # the options are checked before anything runs
    with pytest.raises(ValueError, match="PriorShift.fit: max_iter=1025"):
        ps.fit(ds, max_iter=1025)
    for tol in (-1e-6, float("nan"), float("inf"), "1e-6"):
        with pytest.raises(ValueError, match="PriorShift.fit: tol="):
            ps.fit(ds, tol=tol)
    for priors in ([0.5, 0.5], [0.0] * 4, [0.5, -0.5, 0.5, 0.5], [float("nan")] * 4):
        with pytest.raises(ValueError, match="PriorShift.set_priors: expected 4 finite probabilities"):
            ps.set_priors(priors)
    with pytest.raises(ValueError, match="predict_topk: k=5"):
        ps.predict_topk(ds, k=5)


def test_cli_key_is_validated():
    from slnlp import cli
    assert cli.prior_shift_options(None) is None
    assert cli.prior_shift_options({}) == {"max_iter": 200, "tol": 1e-6, "source": "train"}
    assert cli.prior_shift_options({"max_iter": 0, "tol": 0, "source": "train_labels"}) == {"max_iter": 0, "tol": 0.0, "source": "train_labels"}
    assert cli.prior_shift_options({"tol": "1e-8"}) == {"max_iter": 200, "tol": 1e-8, "source": "train"}      # YAML's reading of 1e-8
    assert "prior_shift" in cli.DICT_ARGS
    for bad, text in (([], "expected a dict"), ({"iters": 3}, "unknown keys"), ({"max_iter": -1}, "max_iter=-1"), ({"max_iter": 1025}, "max_iter=1025"),
                      ({"max_iter": 2.0}, "max_iter=2.0"), ({"max_iter": True}, "max_iter=True"), ({"tol": -1.0}, "tol=-1.0"),
                      ({"tol": float("inf")}, "tol=inf"), ({"tol": "small"}, "tol='small'"), ({"tol": True}, "tol=True"),
                      ({"source": "test"}, "source='test'"), ({"source": None}, "source=None")):
        with pytest.raises(ValueError, match=text):
            cli.prior_shift_options(bad)


def test_ops_fail_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from slnlp import ops
    z = torch.zeros(3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fit_priors(z, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.shift_logp(z, torch.zeros(2, dtype=torch.float64))


def test_the_entry_points_are_declared_and_bound():
    from slnlp import _lib, ops
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    text = src[src.index("label-shift adaptation"):src.index("slnlp_fit_priors_scratch_bytes(int64_t")]
    for said in ("lse_i = max_c a_ic + log sum_c exp(a_ic - max_c a_ic)", "pi^{t+1}_c = S_c / M", "ln max(pi^{t+1}_c, 2^-1022) - log_source_c",
                 "d^t <= tol -> SLNLP_PRIOR_TOL", "t == max_iter -> SLNLP_PRIOR_CAP", "SLNLP_PRIOR_EMPTY", "table double [3, V]",
                 "3 (max_iter + 1) + 2 launches", "No atomics", "rounded once to float32", "NaN\n * in every column"):
        assert said in text, f"the header states the rule so that a caller can restate it: {said!r}"
    for macro, mirror in (("SLNLP_PRIOR_MAX_ITER", _lib.PRIOR_MAX_ITER), ("SLNLP_PRIOR_STATE_BYTES", 8 * ops.PRIOR_STATE_DOUBLES)):
        (found,), = [re.findall(rf"#define {macro}\s+(\d+)", src)]
        assert int(found) == mirror, macro
    for macro, name in (("SLNLP_PRIOR_TOL", "tol"), ("SLNLP_PRIOR_CAP", "cap"), ("SLNLP_PRIOR_EMPTY", "empty")):
        (found,), = [re.findall(rf"#define {macro}\s+(\d+)", src)]
        assert _lib.PRIOR_REASONS[int(found)] == name
    hip = re.sub(r"//.*", "", open(os.path.join(ROOT, "sign-language-nlp_amd", "csrc", "prior_shift.hip")).read())
    assert "atomic" not in hip and "hipMalloc" not in hip and "hipMemcpy" not in hip and "hipStreamSynchronize" not in hip
    assert "csrc/prior_shift.hip" in open(os.path.join(ROOT, "sign-language-nlp_amd", "Makefile")).read()


def test_the_library_checks_its_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    lib = _lib.load()
    # every check comes before the launch, so a machine without a GPU can ask for the codes and messages (the device pointers are
    # never read: they are numbers here)
    N, V = 5, 3
    z, beta, ls, table, state, scratch, out = (k << 20 for k in range(1, 8))
    assert lib.slnlp_fit_priors_scratch_bytes(N, V) == 8 * (2 * N + V)
    assert lib.slnlp_fit_priors_scratch_bytes(0, V) == -1 and b"outside" in lib.slnlp_last_error()
    assert lib.slnlp_fit_priors_scratch_bytes(N, 2 ** 31) == -1

    def fit(**kw):
        a = dict(logp=z, ld=4, N=N, V=V, beta=beta, ls=ls, max_iter=10, tol=1e-6, table=table, state=state, scratch=scratch, bytes=8 * (2 * N + V))
        a.update(kw)
        rc = lib.slnlp_fit_priors(a["logp"], a["ld"], a["N"], a["V"], a["beta"], a["ls"], a["max_iter"], a["tol"], a["table"], a["state"],
                                  a["scratch"], a["bytes"], None)
        return rc, lib.slnlp_last_error().decode()
    big = 2 ** 31
    for kw, text in (({"logp": None}, "null pointer"), ({"ls": None}, "null pointer"), ({"table": None}, "null pointer"),
                     ({"state": None}, "null pointer"), ({"scratch": None}, "null pointer"), ({"N": 0}, "N=0 outside"),
                     ({"N": big}, f"N={big} outside"), ({"V": 0}, "V=0 outside"), ({"V": big, "ld": big}, f"V={big} outside"),
                     ({"ld": 2}, "ld=2 is less than V=3"), ({"max_iter": -1}, "max_iter=-1 outside 0..1024"),
                     ({"max_iter": 1025}, "max_iter=1025 outside 0..1024"), ({"tol": -1.0}, "tol=-1"), ({"tol": float("nan")}, "tol=nan"),
                     ({"tol": float("inf")}, "tol=inf"), ({"bytes": 8 * (2 * N + V) - 8}, "is too small"), ({"logp": z + 2}, "misaligned"),
                     ({"beta": beta + 4}, "misaligned"), ({"ls": ls + 4}, "misaligned"), ({"table": table + 4}, "misaligned"),
                     ({"state": state + 4}, "misaligned"), ({"scratch": scratch + 4}, "misaligned"),
                     ({"table": z + 16}, "output table overlaps input logp"), ({"state": ls + 16}, "output state overlaps input log_source"),
                     ({"scratch": beta}, "output scratch overlaps input beta"), ({"state": table + 64}, "outputs table and state overlap"),
                     ({"scratch": state + 120}, "outputs state and scratch overlap"),
                     ({"table": z + 4 * 18}, "output table overlaps input logp")):       # its last float: 4 rows of 4 floats, then 3
        rc, msg = fit(**kw)
        assert rc == 1 and "fit_priors" in msg and text in msg, (kw, rc, msg)
    assert fit(beta=None, N=0)[1].count("N=0 outside") == 1          # (a null beta is no error: the next check speaks)

    def shift(**kw):
        a = dict(logp=z, ld=4, N=N, V=V, beta=beta, lw=ls, out=out, ld_out=3)
        a.update(kw)
        rc = lib.slnlp_shift_logp(a["logp"], a["ld"], a["N"], a["V"], a["beta"], a["lw"], a["out"], a["ld_out"], None)
        return rc, lib.slnlp_last_error().decode()
    for kw, text in (({"logp": None}, "null pointer"), ({"lw": None}, "null pointer"), ({"out": None}, "null pointer"), ({"N": 0}, "N=0 outside"),
                     ({"V": big, "ld": big, "ld_out": big}, f"V={big} outside"), ({"ld": 2}, "ld=2 is less than V=3"),
                     ({"ld_out": 2}, "ld_out=2 is less than V=3"), ({"logp": z + 2}, "misaligned"), ({"out": out + 2}, "misaligned"),
                     ({"lw": ls + 4}, "misaligned"), ({"beta": beta + 4}, "misaligned"), ({"out": z + 16}, "out overlaps logp without being logp itself"),
                     ({"out": z, "ld_out": 3}, "out overlaps logp without being logp itself"), ({"out": ls - 4}, "out overlaps beta or log_w"),
                     ({"out": beta - 4 * 14}, "out overlaps beta or log_w")):
        rc, msg = shift(**kw)
        assert rc == 1 and "shift_logp" in msg and text in msg, (kw, rc, msg)
