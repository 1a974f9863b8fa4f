"""GPU: ranking metrics on the device -- ``slnlp_ranking_rows`` through the C ABI against the numpy restatement
(tests/ranking_ref.py, itself held to sklearn's binary scorers on the CPU), the scoring names in a fit's history,
``NeuralNetClassifier.ranking`` and ``VotingEnsemble.ranking``.

The bounds: the per-row counts are integers and equal the restatement's; the table's first three columns are exact (counts, and a
sum of integers below 2^53); its fourth column is a sum of P_c terms in (0, 1] whose order alone differs from the restatement's:
within P_c 2^-52 relative; the four scores within 1e-12."""
import numpy as np
import pytest
import torch

from ranking_ref import NAMES, make_scores, ranking_ref

pytestmark = pytest.mark.gpu

BOUND = 1e-12
TEMPERATURE = {"method": "temperature"}
CHUNK = 2048                                                                    # SLNLP_RANK_CHUNK


def _device(z, y, ld=None):
    """``z`` on the device, its rows ``ld`` floats apart (the padding is NaN: never to be read), and the labels."""
    N, V = z.shape
    buf = torch.full((N, ld or V), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(z).cuda()
    return buf[:, :V], torch.from_numpy(np.asarray(y, dtype=np.int64)).cuda()


def _hold(tag, out, z, y):
    """The device's rows and table against the restatement of (z, y); returns the downloaded summary."""
    from slnlp import ops
    rows, table, want = ranking_ref(z, y)
    got_table = out[1].cpu().numpy()
    if out[0] is not None:
        got_rows = out[0].cpu().numpy()
        assert got_rows.dtype == np.int32 and got_rows.shape == rows.shape, tag
        assert np.array_equal(got_rows, rows), (tag, np.flatnonzero((got_rows != rows).any(axis=1))[:8])
    assert got_table.shape == table.shape and np.array_equal(got_table[:, :3], table[:, :3]), tag
    err = np.abs(got_table[:, 3] - table[:, 3])
    print(f"{tag}: max |column 3 - restatement| / (P 2^-52 |restatement|) = "
          f"{np.max(err / np.maximum(table[:, 0] * 2.0 ** -52 * np.abs(table[:, 3]), 1e-300)):.3f}")
    assert (err <= table[:, 0] * 2.0 ** -52 * np.abs(table[:, 3])).all(), tag
    got = ops.ranking_download(out)
    for k in NAMES:
        assert (np.isnan(got[k]) and np.isnan(want[k])) or abs(got[k] - want[k]) <= BOUND, (tag, k, got[k], want[k])
    assert got["classes_scored"] == want["classes_scored"] and np.array_equal(got["support"], want["support"]), tag
    assert np.allclose(got["auc"], want["auc"], rtol=0, atol=BOUND, equal_nan=True), tag
    assert np.allclose(got["ap"], want["ap"], rtol=0, atol=BOUND, equal_nan=True), tag
    return got


def _special():
    z, y = make_scores(130, 6, 9, quantum=0.5)
    z[3, 1], z[40, 1], z[77, 1] = -np.inf, -np.inf, -np.inf                     # -inf: an ordinary value, tied with itself
    z[9, 2], z[10, 2], z[11, 2], z[12, 2] = -0.0, 0.0, -0.0, 0.0                # -0.0 equals +0.0
    y[9], y[10], y[11] = 2, 2, 3
    return z, y


def _kernel_cases():
    one_class, y_one = make_scores(70, 4, 3, quantum=0.5)
    y_one[:] = 2                                                                # every row a positive of class 2: Q = 0 everywhere
    nan, y_nan = make_scores(130, 6, 5, quantum=0.5)
    nan[17, 4] = np.nan                                                         # in a negative's row: class 4 alone is undefined
    bad, y_bad = make_scores(130, 6, 6, quantum=0.5)
    y_bad[3], y_bad[64], y_bad[129] = -1, 6, 2 ** 40
    return [("N1_V1", np.zeros((1, 1), dtype=np.float32), np.array([0]), None),
            ("N5_V3", *make_scores(5, 3, 1), None),
            ("N257_V70_ties", *make_scores(257, 70, 2, quantum=0.25), None),     # N no multiple of 64 or 256, V beyond a wave
            ("N300_V202_absent", *make_scores(300, 202, 4, quantum=0.5, absent=tuple(range(0, 202, 3))), None),
            ("one_class", one_class, y_one, None), ("minus_inf_and_zeros", *_special(), None), ("one_nan", nan, y_nan, None),
            ("bad_labels", bad, y_bad, None), ("N33_V129_ld136", *make_scores(33, 129, 3, quantum=0.5), 136)]


@pytest.mark.parametrize("case", _kernel_cases(), ids=lambda c: c[0])
def test_kernel_against_the_restatement(case):
    from slnlp import ops
    name, z, y, ld = case
    zd, yd = _device(z, y, ld)
    if ld:
        assert zd.stride(0) == ld > z.shape[1]
    got = _hold(name, ops.ranking_rows(zd, yd), z, y)
    table_only = ops.ranking_rows(zd, yd, per_row=False)                         # rows = null
    assert table_only[0] is None
    assert table_only[1].cpu().numpy().tobytes() == ops.ranking_rows(zd, yd)[1].cpu().numpy().tobytes()
    if name == "N1_V1":
        assert got["classes_scored"] == 0 and all(np.isnan(got[k]) for k in NAMES)
    if name == "one_class":
        assert got["classes_scored"] == 0 and got["support"].tolist() == [0, 0, 70, 0]
    if name == "one_nan":
        rows = ops.ranking_rows(zd, yd)[0].cpu().numpy()
        assert got["nan_classes"] == 1 and np.isnan(got["auc"][4]) and got["classes_scored"] == 5
        assert (rows[y == 4, 3] == -2).all() and (rows[y != 4, 3] == 0).all()
    if name == "bad_labels":
        rows = ops.ranking_rows(zd, yd)[0].cpu().numpy()
        assert (got["rows"], got["bad_labels"]) == (127, 3) and rows[[3, 64, 129]].tolist() == [[0, 0, 0, -1]] * 3
    if name == "minus_inf_and_zeros":
        rows = ops.ranking_rows(zd, yd)[0].cpu().numpy()
        assert rows[9, :3].tolist() == rows[10, :3].tolist() and rows[9, 1] >= 1 and rows[9, 2] >= 2       # tied across the zero's two signs


@pytest.mark.parametrize("positives", [CHUNK, CHUNK + 1, 2 * CHUNK + 37])
def test_more_positives_than_one_chunk(positives):
    from slnlp import ops
    N = positives + 300
    z, _ = make_scores(N, 2, positives, quantum=0.125)
    y = np.zeros(N, dtype=np.int64)
    y[np.random.RandomState(positives).permutation(N)[:positives]] = 1
    got = _hold(f"P{positives}", ops.ranking_rows(*_device(z, y)), z, y)
    assert got["support"].tolist() == [300, positives] and got["classes_scored"] == 2


def test_the_result_is_a_pure_function_of_the_arguments():
    from slnlp import ops
    z, y = make_scores(300, 202, 4, quantum=0.5, absent=(5, 6))
    zd, yd = _device(z, y)
    both = lambda out: out[1].cpu().numpy().tobytes() + out[0].cpu().numpy().tobytes()
    out = ops.ranking_buffers(300, 202, "cuda")
    first = ops.ranking_rows(zd, yd, out=out)
    assert first is out
    a = both(out)
    assert both(ops.ranking_rows(zd, yd, out=out)) == a                          # over its own leftovers
    other = (torch.full((300, 4), 7, dtype=torch.int32, device="cuda"), torch.full((203, 4), float("nan"), dtype=torch.float64, device="cuda"))
    assert both(ops.ranking_rows(zd, yd, out=other)) == a
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        elsewhere = ops.ranking_rows(zd, yd)
    side.synchronize()
    assert both(elsewhere) == a


def test_download_is_one_copy(monkeypatch):
    from slnlp import ops
    out = ops.ranking_rows(*_device(*make_scores(257, 70, 2, quantum=0.25)), per_row=False)
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(tuple(t.shape)) or real(t, *a, **k))
    got = ops.ranking_download(out)
    monkeypatch.undo()
    assert copies == [(71, 4)], copies
    assert set(got) == set(NAMES) | {"classes_scored", "auc", "ap", "support", "rows", "bad_labels", "nan_classes"}
    with pytest.raises(ValueError, match="formed no rows"):
        ops.ranking_download(out, per_row=True)


def test_bad_arguments_return_codes_and_messages():
    from slnlp import _lib, ops
    lib = _lib.load()
    z, y = _device(*make_scores(5, 3, 1))
    rows, table = ops.ranking_buffers(5, 3, "cuda")
    p, st = _lib.ptr, _lib.stream_ptr()
    call = lambda *a: (lib.slnlp_ranking_rows(*a, st), lib.slnlp_last_error().decode())
    good = (p(z), 3, p(y), 5, 3, p(rows), p(table))
    for i, value, text in [(0, None, "null pointer"), (2, None, "null pointer"), (6, None, "null pointer"),
                           (3, 0, "N=0"), (3, _lib.RANK_MAX_ROWS + 1, f"N={_lib.RANK_MAX_ROWS + 1}"), (4, 0, "V=0"), (4, 2 ** 31 - 1, "V=2147483647"),
                           (1, 2, "ld=2 is less than V=3"), (1, 2 ** 62, "is no addressable matrix"),
                           (0, p(z) + 2, "misaligned"), (2, p(y) + 4, "misaligned"), (5, p(rows) + 8, "16-byte aligned"),
                           (6, p(table) + 16, "32-byte aligned"), (5, p(table), "rows and table overlap"),
                           (6, p(rows) - 32, "rows and table overlap")]:
        args = list(good)
        args[i] = value
        rc, msg = call(*args)
        assert rc == 1 and text in msg, (i, value, rc, msg)
    big = torch.zeros(64, dtype=torch.float64, device="cuda")                    # an output over an input: nothing is launched
    for i, o, text in [(0, 5, "output rows overlaps input logp"), (2, 5, "output rows overlaps input y"),
                       (0, 6, "output table overlaps input logp"), (2, 6, "output table overlaps input y")]:
        args = list(good)
        args[i], args[o] = p(big), p(big)
        rc, msg = call(*args)
        assert rc == 1 and text in msg, (i, o, rc, msg)
    rc, msg = call(*good[:5], None, good[6])                                     # rows may be null
    assert rc == 0, msg
    torch.cuda.synchronize()                                                    # no sticky error: nothing faulted
    with pytest.raises(ValueError, match="ranking_rows"):
        ops.ranking_rows(z.double(), y)
    with pytest.raises(ValueError, match="ranking_rows"):
        ops.ranking_rows(z, y.int())
    with pytest.raises(ValueError, match="ranking_rows"):
        ops.ranking_rows(z, y, out=(rows, table[:3]))
    with pytest.raises(ValueError, match="ranking_rows"):
        ops.ranking_rows(z, y, out=(rows[:4], table))


def test_epoch_scores_on_device_tensors():
    from slnlp import metrics, ops
    z, y = make_scores(257, 12, 5, quantum=0.25, absent=(3,))
    zd, yd = _device(z, y)
    want = ranking_ref(z, y)[2]
    buf = ops.ranking_buffers(257, 12, "cuda", per_row=False)
    got = metrics.epoch_scores(["accuracy", "auc_macro", "ap_macro"], zd, yd, rank_out=buf)
    assert set(got) == {"accuracy", "auc_macro", "ap_macro"}
    assert abs(got["auc_macro"] - want["auc_macro"]) <= BOUND and abs(got["ap_macro"] - want["ap_macro"]) <= BOUND
    assert got == metrics.epoch_scores(["accuracy", "auc_macro", "ap_macro"], zd, yd)
    yd[4] = 12
    with pytest.raises(ValueError, match="scoring the valid data: 1 of 257 labels lie outside the 12 classes"):
        metrics.epoch_scores(["ap_macro"], zd, yd, split="valid")


# ------------------------------------------------------------------------------------------------------ estimator ----
from test_calibration_gpu import make_net, raw_logp  # noqa: E402

SCORING = ["accuracy", "auc_macro", "ap_macro"]


@pytest.fixture(scope="module")
def ds():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(120, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


@pytest.fixture(scope="module")
def scored(ds):
    """A tiny calibrated fit scored on the two macro names, with every epoch's (split, log-probs, labels) kept."""
    from slnlp import metrics
    net = make_net(ds, max_epochs=2, scoring=SCORING, calibration=TEMPERATURE)
    seen, real = [], metrics.epoch_scores

    def watch(names, logp, y, *a, **k):
        seen.append((k.get("split"), logp.detach().cpu().numpy().copy(), y.detach().cpu().numpy().copy()))
        return real(names, logp, y, *a, **k)
    metrics.epoch_scores = watch
    try:
        net.partial_fit(ds)
    finally:
        metrics.epoch_scores = real
    return net, seen


def _as_given(est, data):
    """The float32 log-probs ``predict_proba`` downloads before the host softmax (calibrated where the estimator is)."""
    keep = est.predict_nonlinearity
    est.predict_nonlinearity = "none"
    try:
        return est.predict_proba(data)
    finally:
        est.predict_nonlinearity = keep


def _check_ranking(got, z, y):
    want = ranking_ref(z, y)[2]
    for k in NAMES:
        assert abs(got[k] - want[k]) <= BOUND, (k, got[k], want[k])
    assert got["classes_scored"] == want["classes_scored"] > 1 and np.array_equal(got["support"], want["support"])
    assert np.allclose(got["auc"], want["auc"], rtol=0, atol=BOUND, equal_nan=True)
    assert np.allclose(got["ap"], want["ap"], rtol=0, atol=BOUND, equal_nan=True)


def test_history_columns_are_the_restatements_on_the_epoch_log_probs(scored):
    net, seen = scored
    assert len(net.history) == 2 and [s[0] for s in seen] == ["train", "valid"] * 2
    for e, row in enumerate(net.history):
        for split, logp, y in seen[2 * e:2 * e + 2]:
            want = ranking_ref(logp, y)[2]
            print(f"epoch {e + 1} {split}: auc_macro {row[f'{split}_auc_macro']:.6f} ap_macro {row[f'{split}_ap_macro']:.6f}")
            assert abs(row[f"{split}_auc_macro"] - want["auc_macro"]) <= BOUND and abs(row[f"{split}_ap_macro"] - want["ap_macro"]) <= BOUND
            assert 0.0 <= row[f"{split}_auc_macro"] <= 1.0 and 0.0 < row[f"{split}_ap_macro"] <= 1.0


def test_ranking_of_a_calibrated_fit(ds, scored):
    net = scored[0]
    assert net.temperature_ != 1.0
    on = net.ranking(ds)
    _check_ranking(on, _as_given(net, ds), ds.y)
    assert on["temperature"] == net.temperature_ and np.array_equal(on["classes"], net.classes_)
    off = net.ranking(ds, calibrated=False)
    _check_ranking(off, raw_logp(net, ds), ds.y)
    assert off["temperature"] == 1.0
    assert net.ranking(ds, y=ds.y)["ap_macro"] == on["ap_macro"]
    wrong = ds.y.copy()
    wrong[3] = len(net.classes_)
    with pytest.raises(ValueError, match="ranking: 1 of 120 labels lie outside the"):
        net.ranking(ds, y=wrong)
    with pytest.raises(ValueError, match="shape"):
        net.ranking(ds, y=ds.y[:5])
    for name in NAMES:
        with pytest.raises(ValueError, match="has no bootstrap interval; known"):
            net.score_interval(ds, scoring=name)


def test_ranking_of_a_two_member_ensemble(ds, scored):
    from slnlp.ensemble import VotingEnsemble
    ens = VotingEnsemble([scored[0], make_net(ds, seed=12, max_epochs=1).partial_fit(ds)])
    got = ens.ranking(ds)
    _check_ranking(got, _as_given(ens, ds), ds.y)
    assert got["temperature"] == 1.0


def test_lockstep_group_matches_solo_fits(ds):
    from slnlp.lockstep import fit_lockstep
    strip = lambda hist: [{k: v for k, v in r.items() if k != "dur"} for r in hist]
    lrs = [0.05, 0.02]
    solo = [make_net(ds, seed=20 + f, lr=lr, max_epochs=2, scoring=SCORING).partial_fit(ds) for f, lr in enumerate(lrs)]
    lock = [make_net(ds, seed=20 + f, lr=lr, max_epochs=2, scoring=SCORING) for f, lr in enumerate(lrs)]
    fit_lockstep(lock, [ds] * 2)
    for f, (a, b) in enumerate(zip(solo, lock)):
        assert all("train_auc_macro" in r and "valid_ap_macro" in r for r in b.history), f
        assert strip(a.history) == strip(b.history), f
        ra, rb = a.ranking(ds), b.ranking(ds)
        assert all(ra[k] == rb[k] for k in NAMES) and np.array_equal(ra["ap"], rb["ap"], equal_nan=True), f
