"""GPU: conformal prediction sets on the device -- ``slnlp_conformal_rows`` / ``_quantile`` / ``_summary`` through the C ABI against
the numpy restatement (tests/conformal_ref.py), ``NeuralNetClassifier.conformalize`` / ``predict_set`` / ``coverage`` and
``VotingEnsemble``'s.

The bounds: ranks, codes, sizes, covered flags and set words are integers and equal the restatement's -- the sets are compared at
a threshold given as an input that every (row, class) score of the restatement stays more than 1e-9 away from, which the test
checks for every row; the scores are sums of at most 1024 terms <= 1, each a few 2^-53 off: within 1e-12 absolute.  The
threshold of the quantile kernel is an order statistic: equal, bit for bit, to ``np.partition`` of the device's own scores."""
import warnings

import numpy as np
import pytest
import torch

import conformal_ref as cr

pytestmark = pytest.mark.gpu

BOUND = 1e-12
MARGIN = 1e-9
CONFIGS = [("lac", dict(method="lac", randomized=False)), ("lac_rand", dict(method="lac", randomized=True, seed=5)),
           ("aps", dict(method="aps", randomized=False)), ("aps_rand", dict(method="aps", randomized=True, seed=7, draw=3)),
           ("raps", dict(method="aps", lam=0.01, k_reg=2, randomized=True, seed=2 ** 63 + 11, draw=1))]


def _device(z, y=None, ld=None):
    """``z`` on the device, its rows ``ld`` floats apart (the padding is NaN: never to be read), and the labels."""
    N, V = z.shape
    buf = torch.full((N, ld or V), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(z).cuda()
    return buf[:, :V], (None if y is None else torch.from_numpy(np.asarray(y, dtype=np.int64)).cuda())


def _threshold(q):
    return torch.tensor([q, 0.0, 0.0, 0.0], dtype=torch.float64).cuda()


def _special():
    z, y = cr.make_logp(12, 9, 8)
    z[0] = -np.inf
    z[0, 4] = 0.0                                                                # p = 1 and the rest -inf
    y[0] = 4
    z[1, 3] = -np.inf                                                            # -inf: an ordinary value, p = 0
    y[1] = 3
    z[2, 6] = np.nan                                                             # code -2
    z[3, 0] = np.inf                                                             # code -2: the maximum is not finite
    z[4, 2], z[4, 5] = -0.0, 0.0                                                 # equal values: by ascending column
    z[5] = -np.inf                                                               # code -2: the maximum is -inf
    return z, y


def _bad_labels():
    z, y = cr.make_logp(20, 6, 6)
    y[3], y[10], y[19] = -1, 6, 2 ** 40
    z[10, 1] = np.nan                                                            # a NaN row with a bad label: the NaN is looked at first
    return z, y


def _cases():
    return [("N1_V1", np.zeros((1, 1), dtype=np.float32), np.array([0]), None, 1.0),
            ("N5_V3", *cr.make_logp(5, 3, 1), None, 1.0),
            ("N257_V64", *cr.make_logp(257, 64, 2), None, 1.0),                  # the sort's padding boundary
            ("N257_V65", *cr.make_logp(257, 65, 3), None, 1.0),
            ("N300_V202", *cr.make_logp(300, 202, 4), None, 1.0),
            ("N33_V129_ld136", *cr.make_logp(33, 129, 5), 136, 1.0),
            ("N9_V1024", *cr.make_logp(9, 1024, 6, lean=4.0), None, 1.0),        # the cap
            ("N64_V70_ties", *cr.make_logp(64, 70, 7, quantum=0.25), None, 1.0),
            ("special_rows", *_special(), None, 1.0),
            ("bad_labels", *_bad_labels(), None, 1.0),
            ("beta_0.5", *cr.make_logp(70, 33, 9), None, 0.5),
            ("beta_2.0", *cr.make_logp(70, 33, 10, quantum=0.25), None, 2.0)]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_kernel_against_the_restatement(case):
    from slnlp import ops
    name, z, y, ld, beta = case
    N, V = z.shape
    zd, yd = _device(z, y, ld)
    if ld:
        assert zd.stride(0) == ld > V
    state = ops.temperature_state(beta, "cuda") if beta != 1.0 else None
    for tag, cfg in CONFIGS:
        S = cr.class_scores(z, beta=beta, **cfg)[0]
        qhat = cr.pick_qhat(S, 0.8, MARGIN)
        want = cr.rows_ref(z, y, qhat=qhat, beta=beta, **cfg)
        assert want["margin"] > MARGIN, (name, tag, want["margin"])              # a condition on the inputs, over every row
        buf = ops.conformal_rows(zd, yd, state=state, qhat=_threshold(qhat), **cfg)
        got = ops.conformal_download(buf, rows=True, sets=True, score=True)
        assert got["rows"].dtype == np.int32 and np.array_equal(got["rows"], want["rows"]), \
            (name, tag, np.flatnonzero((got["rows"] != want["rows"]).any(axis=1))[:8])
        assert np.array_equal(np.isnan(got["score"]), np.isnan(want["score"])), (name, tag)
        err = np.nanmax(np.abs(got["score"] - want["score"])) if not np.isnan(want["score"]).all() else 0.0
        print(f"{name} {tag}: max |score - restatement| = {err:.3e}, qhat {qhat:.6f}, margin {want['margin']:.3e}, "
              f"mean size {want['rows'][:, 0].mean():.2f}")
        assert err <= BOUND, (name, tag, err)
        assert got["sets"].dtype == np.uint32 and np.array_equal(got["sets"], cr.pack_sets(want["mask"])), (name, tag)
        # without labels: the same sets, no rank; without a threshold: the same scores and ranks, no set
        free = ops.conformal_download(ops.conformal_rows(zd, None, state=state, qhat=_threshold(qhat), **cfg), rows=True, sets=True)
        assert np.array_equal(free["sets"], got["sets"]) and np.array_equal(free["rows"][:, 0], got["rows"][:, 0])
        assert not free["rows"][:, 1:3].any() and set(free["rows"][:, 3]) <= {0, -2}
        bare = ops.conformal_download(ops.conformal_rows(zd, yd, state=state, **cfg), rows=True, score=True)
        assert bare["score"].tobytes() == got["score"].tobytes() and np.array_equal(bare["rows"][:, [1, 3]], got["rows"][:, [1, 3]])
        assert not bare["rows"][:, [0, 2]].any()
    if name == "special_rows":
        assert want["rows"][[2, 3, 5], 3].tolist() == [-2, -2, -2] and want["rows"][0, 1] == 1 and want["rows"][1, 1] == V
    if name == "bad_labels":
        assert want["rows"][[3, 10, 19], 3].tolist() == [-1, -2, -1] and want["rows"][3, 0] > 0


def test_top_probability_is_the_reliability_kernels_conf():
    from slnlp import ops
    z, y = cr.make_logp(130, 37, 12, quantum=0.25)
    zd, yd = _device(z, y)
    pred = torch.from_numpy(z.argmax(axis=1).astype(np.int64)).cuda()             # the label of every row: its arg-max
    for state in (None, ops.temperature_state(0.7, "cuda")):
        buf = ops.conformal_rows(zd, pred, method="lac", randomized=False, state=state)
        conf = ops.reliability_rows(zd, pred, state=state)[0][:, 0].cpu().numpy()
        assert ops.conformal_download(buf, score=True)["score"].tobytes() == (1.0 - conf).tobytes()


def _quantile_case(N, alpha, seed, levels=None, excluded=0.1):
    rs = np.random.RandomState(seed)
    score = rs.rand(N) if levels is None else rs.randint(0, levels, size=N) / 4.0
    code = np.where(rs.rand(N) < excluded, rs.choice([-1, -2], size=N), 0)
    score[code != 0] = np.nan
    return score, code, alpha


@pytest.mark.parametrize("case", [("n1_inf", np.array([0.3]), np.array([0]), 0.1), ("n1", np.array([0.3]), np.array([0]), 0.5),
                                  ("N255", *_quantile_case(255, 0.1, 1)), ("N256", *_quantile_case(256, 0.05, 2)),
                                  ("N1000", *_quantile_case(1000, 0.1, 3)), ("N1000_ties", *_quantile_case(1000, 0.2, 4, levels=5)),
                                  ("N1000_signs", _quantile_case(1000, 0.5, 5)[0] - 0.5, _quantile_case(1000, 0.5, 5)[1], 0.5),
                                  ("all_excluded", np.full(40, np.nan), np.full(40, -2), 0.1),
                                  ("k_above_n", *_quantile_case(5, 0.1, 6, excluded=0.0))], ids=lambda c: c[0])
def test_quantile_is_an_exact_order_statistic(case):
    from slnlp import ops
    name, score, code, alpha = case
    N = len(score)
    buf = ops.conformal_buffers(N, 3, "cuda", sets=False)
    buf["score"].copy_(torch.from_numpy(score))
    buf["rows"].zero_()
    buf["rows"][:, 3] = torch.from_numpy(code.astype(np.int32)).cuda()
    assert ops.conformal_quantile(buf, alpha) is buf["state"]
    got = ops.conformal_download(buf, score=True, rows=True)
    mine = got["score"][got["rows"][:, 3] == 0]                                   # the device's own code-0 scores
    qhat, n, k, excluded = cr.quantile_ref(got["score"], got["rows"][:, 3], alpha)
    assert (got["n"], got["k"], got["excluded"]) == (n, k, excluded), (name, got["state"])
    if k > n:
        assert got["qhat"] == np.inf and name in ("n1_inf", "all_excluded", "k_above_n")
    else:
        assert np.float64(got["qhat"]).tobytes() == np.float64(np.partition(mine, k - 1)[k - 1]).tobytes() == np.float64(qhat).tobytes(), name
        assert (mine <= got["qhat"]).sum() >= k > (mine < got["qhat"]).sum()
    other = torch.empty(4, dtype=torch.float64, device="cuda")
    assert ops.conformal_quantile(buf, alpha, state=other) is other and other.cpu().numpy().tobytes() == got["state"].tobytes()


def test_calibrate_then_evaluate_the_same_rows():
    from slnlp import ops
    z, y = cr.make_logp(300, 202, 13)
    zd, yd = _device(z, y)
    buf = ops.conformal_rows(zd, yd, method="aps", randomized=False, draw=0)
    ops.conformal_quantile(buf, 0.1)
    ops.conformal_rows(zd, yd, buf, method="aps", randomized=False, draw=0, qhat=buf["state"])     # the threshold never leaves the device
    ops.conformal_summary(buf, yd)
    got = ops.conformal_download(buf, rows=True, score=True)
    assert (got["n"], got["k"]) == (300, 271)
    covered = int(got["rows"][:, 2].sum())
    assert covered == int((got["score"] <= got["qhat"]).sum()) and covered >= got["k"]
    assert got["table"][:202, 1].sum() == covered


@pytest.mark.parametrize("case", ["plain", "codes"])
def test_summary_table_is_the_restatements(case):
    from slnlp import metrics, ops
    z, y = cr.make_logp(300, 37, 14) if case == "plain" else _bad_labels()
    V = z.shape[1]
    zd, yd = _device(z, y)
    S = cr.class_scores(z, method="aps", randomized=True, seed=3)[0]
    qhat = cr.pick_qhat(S, 0.85, MARGIN)
    want = cr.rows_ref(z, y, qhat=qhat, method="aps", randomized=True, seed=3)
    assert want["margin"] > MARGIN
    buf = ops.conformal_rows(zd, yd, method="aps", randomized=True, seed=3, qhat=_threshold(qhat))
    assert ops.conformal_summary(buf, yd) is buf["table"]
    got = ops.conformal_download(buf)
    table = cr.summary_ref(want["rows"], y, V)
    assert got["table"].dtype == np.int64 and np.array_equal(got["table"], table)
    rep = metrics.conformal_report(got["table"])
    ok = want["rows"][:, 3] == 0
    assert rep["coverage"] == want["rows"][ok, 2].mean() and rep["excluded"] == (~ok).sum() == (0 if case == "plain" else 3)


def test_the_result_is_a_pure_function_of_the_arguments():
    from slnlp import ops
    z, y = cr.make_logp(300, 202, 4, quantum=0.25)
    zd, yd = _device(z, y)
    cfg = dict(method="aps", lam=0.01, k_reg=2, randomized=True, seed=9, draw=1)
    q = _threshold(0.93)

    def run(buf=None):
        buf = ops.conformal_rows(zd, yd, buf, qhat=q, **cfg)
        ops.conformal_quantile(buf, 0.1)
        ops.conformal_summary(buf, yd)
        return buf
    everything = lambda buf: buf["flat"].cpu().numpy().tobytes()
    out = run()
    a = everything(out)
    assert run(out) is out and everything(out) == a                              # over its own leftovers
    poisoned = ops.conformal_buffers(300, 202, "cuda")
    poisoned["flat"].fill_(0x7F7F7F7F7F7F7F7F)
    run(poisoned)
    for key in ("state", "table", "score", "rows", "sets"):
        assert poisoned[key].cpu().numpy().tobytes() == out[key].cpu().numpy().tobytes(), key
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        elsewhere = run()
    side.synchronize()
    for key in ("state", "table", "score", "rows", "sets"):
        assert elsewhere[key].cpu().numpy().tobytes() == out[key].cpu().numpy().tobytes(), key


def test_download_is_one_copy_of_state_and_table(monkeypatch):
    from slnlp import ops
    z, y = cr.make_logp(257, 70, 2)
    zd, yd = _device(z, y)
    buf = ops.conformal_rows(zd, yd, qhat=_threshold(0.9))
    ops.conformal_quantile(buf, 0.1)
    ops.conformal_summary(buf, yd)
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(tuple(t.shape)) or real(t, *a, **k))
    got = ops.conformal_download(buf)
    assert copies == [(4 + 4 * 71,)], copies
    ops.conformal_download(buf, rows=True, sets=True)
    monkeypatch.undo()
    assert copies[1:] == [(4 + 4 * 71,), (257, 4), (257, 3)], copies
    assert set(got) == {"state", "table", "qhat", "n", "k", "excluded"}
    with pytest.raises(ValueError, match="hold none"):
        ops.conformal_download(ops.conformal_rows(zd, yd), sets=True)


def test_bad_arguments_return_codes_and_messages():
    from slnlp import _lib, ops
    lib = _lib.load()
    z, y = _device(*cr.make_logp(5, 3, 1))
    buf = ops.conformal_buffers(5, 3, "cuda")
    q, beta = _threshold(0.9), ops.temperature_state(1.0, "cuda")
    p, st = _lib.ptr, _lib.stream_ptr()
    call = lambda *a: (lib.slnlp_conformal_rows(*a, st), lib.slnlp_last_error().decode())
    #       0     1   2     3  4  5        6  7    8  9  10 11 12    13                14               15
    good = (p(z), 3, p(y), 5, 3, p(beta), 1, 0.0, 0, 1, 0, 0, p(q), p(buf["score"]), p(buf["rows"]), p(buf["sets"]))
    assert call(*good)[0] == 0
    for i, value, text in [(0, None, "null pointer"), (3, 0, "N=0"), (3, 2 ** 31, "N=2147483648"), (4, 0, "V=0"), (4, 1025, "V=1025"),
                           (1, 2, "ld=2 is less than V=3"), (1, 2 ** 62, "is no addressable matrix"), (6, 2, "method=2"), (6, -1, "method=-1"),
                           (7, -0.5, "lam=-0.5"), (7, float("inf"), "lam=inf"), (7, float("nan"), "lam=nan"), (8, -1, "k_reg=-1"),
                           (2, None, "score needs y"), (12, None, "sets needs qhat_dev"),
                           (0, p(z) + 2, "misaligned"), (2, p(y) + 4, "misaligned"), (5, p(beta) + 4, "misaligned"), (12, p(q) + 4, "misaligned"),
                           (13, p(buf["score"]) + 4, "misaligned"), (15, p(buf["sets"]) + 2, "misaligned"),
                           (14, p(buf["rows"]) + 8, "16-byte aligned"), (14, p(buf["score"]), "outputs score and rows overlap"),
                           (15, p(buf["rows"]) + 16, "outputs rows and sets overlap"), (15, p(buf["score"]) + 8, "outputs score and sets overlap")]:
        args = list(good)
        args[i] = value
        rc, msg = call(*args)
        assert rc == 1 and text in msg, (i, value, rc, msg)
    big = torch.zeros(64, dtype=torch.float64, device="cuda")                    # an output over an input: nothing is launched
    for i, o, text in [(0, 13, "output score overlaps input logp"), (2, 14, "output rows overlaps input y"),
                       (5, 15, "output sets overlaps input beta"), (12, 13, "output score overlaps input qhat"),
                       (0, 15, "output sets overlaps input logp")]:
        args = list(good)
        args[i], args[o] = p(big), p(big)
        rc, msg = call(*args)
        assert rc == 1 and text in msg, (i, o, rc, msg)
    for drop in [(2, 13), (5,), (12, 15), (13,), (14,), (15,), (2, 12, 13, 14, 15)]:          # what may be null
        args = list(good)
        for i in drop:
            args[i] = None
        rc, msg = call(*args)
        assert rc == 0, (drop, msg)
    quant = lambda *a: (lib.slnlp_conformal_quantile(*a, st), lib.slnlp_last_error().decode())
    good_q = (p(buf["score"]), p(buf["rows"]), 5, 0.1, p(buf["state"]))
    assert quant(*good_q)[0] == 0
    for i, value, text in [(0, None, "null pointer"), (1, None, "null pointer"), (4, None, "null pointer"), (2, 0, "N=0"),
                           (3, 0.0, "alpha=0 outside (0, 1)"), (3, 1.0, "alpha=1 outside (0, 1)"), (3, float("nan"), "alpha=nan"),
                           (0, p(buf["score"]) + 4, "misaligned"), (1, p(buf["rows"]) + 8, "16-byte aligned"),
                           (4, p(buf["state"]) + 16, "32-byte aligned"), (4, p(buf["rows"]) - (p(buf["rows"]) % 32), "output state overlaps input")]:
        args = list(good_q)
        args[i] = value
        rc, msg = quant(*args)
        assert rc == 1 and text in msg, (i, value, rc, msg)
    summ = lambda *a: (lib.slnlp_conformal_summary(*a, st), lib.slnlp_last_error().decode())
    good_s = (p(buf["rows"]), p(y), 5, 3, p(buf["table"]))
    assert summ(*good_s)[0] == 0
    for i, value, text in [(0, None, "null pointer"), (1, None, "null pointer"), (4, None, "null pointer"), (2, 0, "N=0"), (3, 0, "V=0"),
                           (3, 1025, "V=1025"), (1, p(y) + 4, "misaligned"), (0, p(buf["rows"]) + 4, "16-byte aligned"),
                           (4, p(buf["table"]) + 8, "32-byte aligned"), (0, p(buf["table"]), "output table overlaps input rows")]:
        args = list(good_s)
        args[i] = value
        rc, msg = summ(*args)
        assert rc == 1 and text in msg, (i, value, rc, msg)
    torch.cuda.synchronize()                                                    # no sticky error: nothing faulted
    with pytest.raises(ValueError, match="conformal_rows"):
        ops.conformal_rows(z.double(), y)
    with pytest.raises(ValueError, match="conformal_rows"):
        ops.conformal_rows(z, y.int())
    with pytest.raises(ValueError, match="conformal_rows: method"):
        ops.conformal_rows(z, y, method="raps")
    with pytest.raises(ValueError, match="conformal_rows: buf"):
        ops.conformal_rows(z, y, ops.conformal_buffers(4, 3, "cuda"))
    with pytest.raises(ValueError, match="conformal_rows: qhat"):
        ops.conformal_rows(z, y, qhat=torch.zeros(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="1025 classes"):
        ops.conformal_rows(torch.zeros(2, 1025, device="cuda"), None)


# ------------------------------------------------------------------------------------------------------ estimator ----
from test_calibration_gpu import make_net, raw_logp  # noqa: E402

TEMPERATURE = {"method": "temperature"}
OPTION = {"alpha": 0.2, "seed": 5}


@pytest.fixture(scope="module")
def ds():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(120, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


@pytest.fixture(scope="module")
def fitted(ds):
    """A tiny calibrated fit whose ``conformal`` option took the threshold on its valid split."""
    return make_net(ds, max_epochs=2, calibration=TEMPERATURE, conformal=OPTION).partial_fit(ds)


def _sets_of(est, z, beta):
    """The restatement of ``predict_set`` on the log-probs ``z`` at ``beta`` under ``est.conformal_``."""
    c = est.conformal_
    cfg = dict(method=c["method"], lam=c["lam"], k_reg=c["k_reg"], randomized=c["randomized"], seed=c["seed"], draw=1, beta=beta)
    want = cr.rows_ref(z, None, qhat=c["qhat"], **cfg)
    assert want["margin"] > MARGIN
    order = cr.probs_and_order(z, beta)[1]
    return want, [order[i, :want["rows"][i, 0]] for i in range(len(z))]


def test_the_option_sets_the_threshold_on_the_valid_split(ds, fitted):
    net = fitted
    c = net.conformal_
    assert {k: c[k] for k in ("alpha", "method", "randomized", "lam", "k_reg", "seed")} == \
        {"alpha": 0.2, "method": "aps", "randomized": True, "lam": 0.0, "k_reg": 0, "seed": 5}
    va = ds[net._train_split(ds)[1]]
    assert c["calibrated"] is True and c["n"] == len(va) == 24 and c["k"] == 20 and c["excluded"] == 0 and 0.0 < c["qhat"] < 2.0
    cal = cr.rows_ref(raw_logp(net, va), va.y, beta=net.calibration_["beta"], method="aps", randomized=True, seed=5, draw=0)
    assert abs(c["qhat"] - cr.quantile_ref(cal["score"], cal["rows"][:, 3], 0.2)[0]) <= BOUND
    assert net._conf_state.is_cuda and net._conf_state.cpu().numpy()[0] == c["qhat"]


def test_predict_set_is_the_restatement_on_the_downloaded_log_probs(ds, fitted):
    net = fitted
    assert net.temperature_ != 1.0
    want, lists = _sets_of(net, raw_logp(net, ds), net.calibration_["beta"])
    got = net.predict_set(ds, return_mask=True)
    assert got["sets"].dtype == bool and np.array_equal(got["sets"], want["mask"]) and np.array_equal(got["sizes"], want["rows"][:, 0])
    listed = net.predict_set(ds)
    assert np.array_equal(listed["sizes"], got["sizes"]) and len(listed["sets"]) == len(ds)
    assert all(np.array_equal(a, net.classes_[b]) for a, b in zip(listed["sets"], lists))
    rep = net.coverage(ds)
    covered = want["mask"][np.arange(len(ds)), ds.y]
    print(f"coverage {rep['coverage']:.4f} mean size {rep['mean_size']:.3f} qhat {rep['qhat']:.4f}")
    assert rep["coverage"] == covered.mean() and rep["mean_size"] == got["sizes"].mean() and rep["rows"] == len(ds)
    assert np.array_equal(rep["size_hist"], np.bincount(got["sizes"], minlength=len(net.classes_) + 1)) and rep["alpha"] == 0.2 and rep["k"] == 20
    assert net.coverage(ds, y=ds.y)["coverage"] == rep["coverage"]
    wrong = ds.y.copy()
    wrong[3] = len(net.classes_)
    with pytest.raises(ValueError, match="coverage: 1 of 120 labels lie outside the"):
        net.coverage(ds, y=wrong)
    with pytest.raises(ValueError, match="conformalize: 1 of 120 labels lie outside the"):
        net.conformalize(ds, y=wrong)


def test_calibrated_and_uncalibrated_paths_differ(ds, fitted):
    net = fitted
    before = dict(net.conformal_), net._conf_state
    try:
        net.conformalize(ds, alpha=0.2, seed=5, calibrated=False)
        assert net.conformal_["calibrated"] is False and net.conformal_["n"] == 120 and net.conformal_["k"] == 97
        want = _sets_of(net, raw_logp(net, ds), 1.0)[0]
        off = net.predict_set(ds, return_mask=True)
        assert np.array_equal(off["sets"], want["mask"])
        net.conformalize(ds, alpha=0.2, seed=5)
        assert net.conformal_["calibrated"] is True
        on = net.predict_set(ds, return_mask=True)
        assert np.array_equal(on["sets"], _sets_of(net, raw_logp(net, ds), net.calibration_["beta"])[0]["mask"])
        assert not np.array_equal(on["sets"], off["sets"])
        # the other options reach the kernel too (randomised: a deterministic score of a calibration row, or of its duplicate in this
        # small synthetic set, IS the threshold, and no margin separates the two sides there)
        net.conformalize(ds[np.arange(0, 120, 2)], alpha=0.2, lam=0.01, k_reg=1, seed=8)
        assert net.conformal_["n"] == 60 and net.conformal_["k"] == 49 and net.conformal_["lam"] == 0.01
        assert np.array_equal(net.predict_set(ds, return_mask=True)["sets"], _sets_of(net, raw_logp(net, ds), net.calibration_["beta"])[0]["mask"])
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            net.conformalize(ds[np.arange(3)], alpha=0.1)
        assert net.conformal_["qhat"] == np.inf and net.conformal_["n"] == 3 and any("at least 9 rows" in str(w.message) for w in seen)
        assert net.predict_set(ds, return_mask=True)["sets"].all()
    finally:
        net.conformal_, net._conf_state = before


def test_save_and_load_round_trip(ds, fitted, tmp_path):
    net = fitted
    net.save_params(str(tmp_path))
    back = make_net(ds, max_epochs=2, calibration=TEMPERATURE, conformal=OPTION)
    with pytest.raises(RuntimeError, match="no threshold yet"):
        back.predict_set(ds)
    back.load_params(str(tmp_path))
    back.classes_ = net.classes_
    assert back.conformal_ == net.conformal_ and back._conf_state.cpu().numpy()[0] == net.conformal_["qhat"]
    a, b = net.predict_set(ds, return_mask=True), back.predict_set(ds, return_mask=True)
    assert np.array_equal(a["sets"], b["sets"]) and np.array_equal(a["sizes"], b["sizes"])


def test_two_member_ensemble(ds, fitted):
    from slnlp.ensemble import VotingEnsemble
    ens = VotingEnsemble([fitted, make_net(ds, seed=12, max_epochs=1).partial_fit(ds)])
    with pytest.raises(RuntimeError, match="no threshold yet"):
        ens.predict_set(ds)
    assert ens.conformalize(ds, alpha=0.2, seed=3) is ens and ens.conformal_["calibrated"] is False and ens.conformal_["n"] == 120
    keep = ens.predict_nonlinearity
    ens.predict_nonlinearity = "none"
    try:
        z = ens.predict_proba(ds)
    finally:
        ens.predict_nonlinearity = keep
    cal = cr.rows_ref(z, ds.y, method="aps", randomized=True, seed=3, draw=0)
    assert abs(ens.conformal_["qhat"] - cr.quantile_ref(cal["score"], cal["rows"][:, 3], 0.2)[0]) <= BOUND
    want = _sets_of(ens, z, 1.0)[0]
    got = ens.predict_set(ds, return_mask=True)
    assert np.array_equal(got["sets"], want["mask"])
    rep = ens.coverage(ds)
    assert rep["coverage"] == want["mask"][np.arange(len(ds)), ds.y].mean() and rep["coverage"] >= 0.65


def test_lockstep_group_matches_solo_fits(ds):
    from slnlp.lockstep import fit_lockstep
    lrs = [0.05, 0.02]
    kw = dict(max_epochs=2, calibration=TEMPERATURE, conformal=OPTION)
    solo = [make_net(ds, seed=20 + f, lr=lr, **kw).partial_fit(ds) for f, lr in enumerate(lrs)]
    lock = [make_net(ds, seed=20 + f, lr=lr, **kw) for f, lr in enumerate(lrs)]
    fit_lockstep(lock, [ds] * 2)
    for f, (a, b) in enumerate(zip(solo, lock)):
        assert a.conformal_ == b.conformal_ and a.conformal_["n"] == 24, f
        assert np.array_equal(a.predict_set(ds, return_mask=True)["sets"], b.predict_set(ds, return_mask=True)["sets"]), f
    assert solo[0].conformal_["qhat"] != solo[1].conformal_["qhat"]
