"""GPU: the label audit on the device -- ``slnlp_label_audit`` and ``slnlp_scatter_logp`` through the C ABI against the numpy
restatement (tests/label_audit_ref.py), ``slnlp.cross_fit`` / ``slnlp.OutOfFold`` and ``LogProbJudge.label_issues`` on fits.

The bounds.  pred, k, code, flags, n_c, the joint, its overflow cell, the pairs and the counts are integers and equal the
restatement's.  That comparison is honest only where no probability lies at its class's threshold, so every case ASSERTS, as a
condition on its inputs, that in the restatement every |p_ic - t_c| exceeds 1e-9 -- except for the (row, own class) pair of a
single-row class, where equality is exact by the definition and must yield "confident".  s, other and m are probabilities from
the shared row head: within the project's 1e-12 absolute.  t_c is a mean of n_c such terms <= 1, added in a fixed order: within
1e-12 + n_c 2^-53 of the restatement's ``math.fsum``.  The tests print the measured maxima; DESIGN.md section 4 records them."""
import numpy as np
import pytest
import torch

import conformal_ref as cr
import label_audit_ref as lr

pytestmark = pytest.mark.gpu

BOUND, MARGIN, LEAN = 1e-12, 1e-9, 3.0
SENTINEL = 0x5A5A5A5A


def _device(z, y=None, ld=None):
    """``z`` on the device, its rows ``ld`` floats apart (the padding is NaN: never to be read), and the labels."""
    N, V = z.shape
    buf = torch.full((N, ld or V), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(z).cuda()
    return buf[:, :V], (None if y is None else torch.from_numpy(np.asarray(y, dtype=np.int64)).cuda())


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
    z[6, 1] = z[6, 7] = z[6].max() + 1.0                                         # two columns at the maximum
    return z, y


def _bad_labels():
    z, y = cr.make_logp(20, 6, 6)
    y[3], y[10], y[19] = -1, 6, 2 ** 40
    z[10, 1] = np.nan                                                            # a NaN row with a bad label: the NaN is looked at first
    return z, y


def _cases():
    mk = lambda *a, **k: cr.make_logp(*a, lean=LEAN, **k)
    return [("N1_V1", np.zeros((1, 1), dtype=np.float32), np.array([0]), None, 1.0),
            ("N5_V3", *mk(5, 3, 1), None, 1.0),
            ("N70_V63", *mk(70, 63, 2), None, 1.0),                              # one short of a wave
            ("N70_V64", *mk(70, 64, 3), None, 1.0),
            ("N70_V65", *mk(70, 65, 4), None, 1.0),
            ("N300_V202", *mk(300, 202, 5), None, 1.0),                          # the data set's classes: empty and single-row ones
            ("N33_V129_ld136", *mk(33, 129, 6), 136, 1.0),
            ("N64_V70_ties", *mk(64, 70, 7, quantum=0.25), None, 1.0),
            ("beta_0.5", *mk(70, 33, 9), None, 0.5),
            ("beta_2.0", *mk(70, 33, 10, quantum=0.25), None, 2.0),
            ("N255_V7", *mk(255, 7, 11), None, 1.0),                             # around the 256-thread tree of the class sums
            ("N256_V7", *mk(256, 7, 12), None, 1.0),
            ("N257_V7", *mk(257, 7, 13), None, 1.0),
            ("N1025_V5", *mk(1025, 5, 14), None, 1.0),
            ("N2100_V9", *mk(2100, 9, 15), None, 1.0),
            ("special_rows", *_special(), None, 1.0),
            ("bad_labels", *_bad_labels(), None, 1.0)]


def _audit(zd, yd, beta=1.0, pairs=20, per_row=True):
    from slnlp import ops
    state = ops.temperature_state(beta, "cuda") if beta != 1.0 else None
    buf = ops.label_audit_buffers(zd.shape[0], zd.shape[1], pairs, "cuda")
    buf["flat"].fill_(SENTINEL)
    assert ops.label_audit_rows(zd, yd, buf, state=state) is buf
    return ops.label_audit_download(buf, per_row=per_row), buf, state


def _same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def _err(a, b):
    ok = ~np.isnan(b)
    return float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_kernels_against_the_restatement(case):
    from slnlp import ops
    name, z, y, ld, beta = case
    N, V = z.shape
    want = lr.audit_ref(z, y, beta=beta)
    gap = lr.smallest_gap(want, y)
    assert gap > MARGIN, (name, gap)                                             # the condition on the inputs (change the seed, not the margin)
    zd, yd = _device(z, y, ld)
    if ld:
        assert zd.stride(0) == ld > V
    got, buf, state = _audit(zd, yd, beta)
    for key in ("pred", "k", "code", "flags"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (name, key, np.flatnonzero(got[key] != want[key])[:8])
    assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["joint"], want["joint"]) and got["overflow"] == want["overflow"]
    M = len(want["pairs"])
    assert [tuple(p) for p in got["pairs"][:M].tolist()] == want["pairs"] and (got["pairs"][M:] == [-1, -1, 0]).all()
    c = want["counts"]
    assert got["head"].tolist() == [c["usable"], c["bad_labels"], c["nan_rows"], c["unconfident"], c["issues"], c["argmax_disagrees"], 0, 0]
    for key in ("s", "other", "m", "p_pred", "t"):
        assert _same_nan(got[key], want[key]), (name, key)
    errs = {key: _err(got[key], want[key]) for key in ("s", "other", "m", "p_pred")}
    t_bound = BOUND + want["n"] * 2.0 ** -53
    has = want["n"] > 0
    t_excess = float((np.abs(got["t"][has] - want["t"][has]) / t_bound[has]).max()) if has.any() else 0.0
    single = np.flatnonzero((want["code"] == 0) & (want["n"][np.clip(y, 0, V - 1)] == 1))
    print(f"{name}: smallest |p - t| {gap:.3e}; max error s {errs['s']:.3e} other {errs['other']:.3e} m {errs['m']:.3e} p_pred {errs['p_pred']:.3e} "
          f"(bound {BOUND:.0e}); t error / bound {t_excess:.2e}; {c['issues']} issues, {c['unconfident']} unconfident, {single.size} single-row "
          f"classes, noise pairs {M}")
    assert max(errs.values()) <= BOUND and t_excess <= 1.0, (name, errs, t_excess)
    # a single-row class: its threshold is its row's own s bit for bit, and the row is confidently its own class or a likelier one
    for i in single:
        assert got["t"][y[i]] == got["s"][i] and got["k"][i] >= 0
    assert (got["m"][want["code"] == 0] == (got["s"] - got["other"])[want["code"] == 0]).all()
    # the same statements as topk_rows: the same bits
    top_idx, top_p = ops.topk_download(ops.topk_rows(zd, min(2, V), state=state))
    assert np.array_equal(got["pred"], top_idx[:, 0]) and got["p_pred"][want["code"] != -2].tobytes() == top_p[want["code"] != -2, 0].tobytes()
    hit = (want["code"] == 0) & (want["pred"] == y)
    assert got["s"][hit].tobytes() == top_p[hit, 0].tobytes()
    if V >= 2:
        assert got["other"][hit].tobytes() == top_p[hit, 1].tobytes()            # the runner-up of a row labelled with its arg-max
    # without the per-row extras the copy ends with the flags and carries the same values
    lean = ops.label_audit_download(buf)
    assert set(lean) == set(got) - {"pred", "other", "p_pred"} and all(np.asarray(lean[q]).tobytes() == np.asarray(got[q]).tobytes() for q in lean)
    if name == "special_rows":
        assert want["code"].tolist() == [0, 0, -2, -2, 0, -2, 0, 0, 0, 0, 0, 0] and got["s"][0] == 1.0 and got["s"][1] == 0.0
        assert got["k"][[2, 3, 5]].tolist() == [-1, -1, -1] and not got["flags"][[2, 3, 5]].any()
    if name == "bad_labels":
        assert want["code"][[3, 10, 19]].tolist() == [-1, -2, -1] and got["k"][[3, 10, 19]].tolist() == [-1, -1, -1]
        assert not np.isnan(got["p_pred"][[3, 19]]).any() and np.isnan(got["p_pred"][10])
    if name == "N1_V1":
        assert (got["s"][0], got["other"][0], got["m"][0], got["t"][0], got["k"][0], got["flags"][0]) == (1.0, 0.0, 1.0, 1.0, 0, 0)


def test_the_audit_is_a_pure_function_of_the_arguments():
    from slnlp import _lib, ops
    z, y = cr.make_logp(1025, 37, 21, lean=LEAN)
    zd, yd = _device(z, y)
    a, buf, _ = _audit(zd, yd)
    b, _, _ = _audit(zd, yd)
    wide, _ = _device(z, None, 41)
    c, _, _ = _audit(wide, yd)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d, _, _ = _audit(zd, yd)
    side.synchronize()
    for other in (b, c, d):
        for key in a:
            assert np.asarray(a[key]).tobytes() == np.asarray(other[key]).tobytes(), key
    # exactly the documented bytes are written: a sentinel-filled tail behind them stays, and one byte less is refused
    end = buf["end"]
    flat = torch.full((end + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    args = (_lib.ptr(zd), zd.stride(0), _lib.ptr(yd), 1025, 37, None, 20, _lib.ptr(flat))
    assert lib.slnlp_label_audit(*args, end * 4, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (flat[end:] == SENTINEL).all() and flat[:buf["at"]["work"]].cpu().numpy().tobytes() == buf["flat"][:buf["at"]["work"]].cpu().numpy().tobytes()
    assert lib.slnlp_label_audit(*args, end * 4 - 1, _lib.stream_ptr()) == 1 and "is too small" in lib.slnlp_last_error().decode()


def test_one_download(monkeypatch):
    from slnlp import ops
    z, y = cr.make_logp(300, 37, 14, lean=LEAN)
    zd, yd = _device(z, y)
    buf = ops.label_audit_rows(zd, yd, pairs=5)
    for per_row, a_row in ((False, 28), (True, 48)):
        copies, real = [], torch.Tensor.cpu
        monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(t.numel() * t.element_size()) or real(t, *a, **k))
        ops.label_audit_download(buf, per_row=per_row)
        monkeypatch.undo()
        assert len(copies) == 1 and copies[0] <= 64 + 37 * 12 + (37 * 37 + 1) * 4 + 60 + 300 * a_row + 64, (per_row, copies)


# -------------------------------------------------------------------------------------------------------- scatter ----
@pytest.mark.parametrize("beta", [None, 0.5, 2.0])
def test_scatter_logp_is_scale_logp_row_by_row(beta):
    from slnlp import ops
    state = None if beta is None else ops.temperature_state(beta, "cuda")
    for n, V, ld, ld_out, N_out in [(1, 5, None, None, 3), (7, 63, None, 70, 7), (70, 65, 72, None, 100), (300, 202, 205, 208, 777)]:
        z, _ = cr.make_logp(n, V, 30 + n)
        zd, _ = _device(z, None, ld)
        rows = np.random.RandomState(n).permutation(N_out)[:n].astype(np.int64)
        base = torch.full((N_out, ld_out or V), float("nan"), dtype=torch.float32, device="cuda")
        out = base[:, :V]
        assert ops.scatter_logp(zd, torch.from_numpy(rows).cuda(), out, state=state) is out
        want = z if beta is None else ops.scale_logp(zd, state).cpu().numpy()
        got = out.cpu().numpy()
        assert got[rows].tobytes() == want.tobytes(), (beta, n, V)                # bit for bit
        rest = np.setdiff1d(np.arange(N_out), rows)
        assert np.isnan(got[rest]).all()                                          # rows not named keep their fill
        if ld_out:
            assert torch.isnan(base[:, V:]).all()                                 # so does the padding
        if beta is not None:
            assert np.abs(want.astype(np.float64) - lr.scale_ref(z, beta)).max() <= 2e-6
    # an index outside the output is skipped, never used as an address
    z, _ = cr.make_logp(4, 6, 1)
    zd, _ = _device(z)
    out = torch.full((3, 6), float("nan"), dtype=torch.float32, device="cuda")
    ops.scatter_logp(zd, torch.tensor([2, -1, 3, 2 ** 40], dtype=torch.int64).cuda(), out, state=state)
    got = out.cpu().numpy()
    assert np.isnan(got[:2]).all() and not np.isnan(got[2]).any()


def test_bad_arguments_return_codes_and_messages():
    from slnlp import _lib, ops
    lib = _lib.load()
    z, y = _device(*cr.make_logp(5, 3, 1))
    buf = ops.label_audit_buffers(5, 3, 4, "cuda")
    flat, beta = buf["flat"], ops.temperature_state(1.0, "cuda")
    p, st = _lib.ptr, _lib.stream_ptr()
    call = lambda *a: (lib.slnlp_label_audit(*a, st), lib.slnlp_last_error().decode())
    #       0     1   2     3  4  5        6  7        8
    good = (p(z), 3, p(y), 5, 3, p(beta), 4, p(flat), flat.numel() * 4)
    assert call(*good)[0] == 0
    for i, value, text in [(0, None, "null pointer"), (2, None, "null pointer"), (7, None, "null pointer"), (3, 0, "N=0"), (3, 2 ** 31, "N=2147483648"),
                           (4, 0, "V=0"), (4, 4097, "V=4097"), (1, 2, "ld=2 is less than V=3"), (1, 2 ** 62, "is no addressable matrix"),
                           (6, 0, "M=0"), (6, 65, "M=65"), (8, 8, "is too small"), (8, -1, "is too small"),
                           (0, p(z) + 2, "misaligned"), (2, p(y) + 4, "misaligned"), (5, p(beta) + 4, "misaligned"), (7, p(flat) + 4, "misaligned"),
                           (7, p(z), "output buf overlaps input logp"), (7, p(y), "output buf overlaps input y"),
                           (5, p(flat) + 64, "output buf overlaps input beta")]:
        args = list(good)
        args[i] = value
        rc, msg = call(*args)
        assert rc == 1 and "label_audit" in msg and text in msg, (i, value, rc, msg)
    args = list(good)
    args[5] = None                                                               # what may be null
    assert call(*args)[0] == 0
    rows = torch.tensor([4, 0, 2, 1, 3], dtype=torch.int64).cuda()
    out = torch.zeros(6, 4, dtype=torch.float32, device="cuda")
    scatter = lambda *a: (lib.slnlp_scatter_logp(*a, st), lib.slnlp_last_error().decode())
    #         0     1   2  3  4        5        6       7  8
    good_s = (p(z), 3, 5, 3, p(beta), p(rows), p(out), 4, 6)
    assert scatter(*good_s)[0] == 0
    for i, value, text in [(0, None, "null pointer"), (5, None, "null pointer"), (6, None, "null pointer"), (2, 0, "N=0"), (3, 0, "V=0"),
                           (1, 2, "ld=2 is less than V=3"), (7, 2, "ld_out=2 is less than V=3"), (7, 2 ** 62, "is no addressable matrix"),
                           (8, 0, "N_out=0"), (8, 2 ** 31, "N_out=2147483648"), (0, p(z) + 2, "misaligned"), (6, p(out) + 2, "misaligned"),
                           (4, p(beta) + 4, "misaligned"), (5, p(rows) + 4, "misaligned"), (6, p(z), "output out overlaps input logp"),
                           (6, p(rows), "output out overlaps input rows"), (4, p(out) + 8, "output out overlaps input beta")]:
        args = list(good_s)
        args[i] = value
        rc, msg = scatter(*args)
        assert rc == 1 and "scatter_logp" in msg and text in msg, (i, value, rc, msg)
    args = list(good_s)
    args[4] = None
    assert scatter(*args)[0] == 0
    torch.cuda.synchronize()                                                    # no sticky error: nothing faulted
    with pytest.raises(ValueError, match="label_audit_rows"):
        ops.label_audit_rows(z.double(), y)
    with pytest.raises(ValueError, match="label_audit_rows"):
        ops.label_audit_rows(z, y.int())
    with pytest.raises(ValueError, match="label_audit_rows: buf must be"):
        ops.label_audit_rows(z, y, ops.label_audit_buffers(6, 3, 4, "cuda"))
    with pytest.raises(ValueError, match="label_audit_buffers: pairs"):
        ops.label_audit_buffers(5, 3, 65, "cuda")
    with pytest.raises(ValueError, match="scatter_logp: rows"):
        ops.scatter_logp(z, rows.int(), out[:, :3])
    with pytest.raises(ValueError, match="scatter_logp: out"):
        ops.scatter_logp(z, rows, out)


# ------------------------------------------------------------------------------------------------------ estimator ----
GRU = dict(module="model.EncoderDecoderGRUAttn", module__embedding_size=24, module__hidden_size=32, module__num_layers=2)


def make_net(ds, **kw):
    """The tiny GRU estimator of tests/test_prior_shift_gpu.py, not initialised: ``cross_fit`` clones and fits it."""
    from slnlp.net import NeuralNetClassifier
    args = dict(module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y, module__batch_first=True, **GRU,
                criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1, optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05,
                max_epochs=2, batch_size=20, device="cuda", gradient_clipping={"gradient_clip_value": 0.5})
    args.update(kw)
    return NeuralNetClassifier(**args)


def _noisy_labels(data, V):
    rs = np.random.RandomState(0)
    y = np.asarray(data.y, dtype=np.int64)
    return np.where(rs.rand(len(y)) < 0.3, rs.randint(0, V, size=len(y)), y)


def _raw(est, ds):
    """The float32 log-probs ``predict_proba`` downloads, before the host softmax."""
    est.predict_nonlinearity = "none"                        # shadows a fit's parameter / a wrapper's class attribute
    try:
        return est.predict_proba(ds)
    finally:
        del est.predict_nonlinearity


@pytest.fixture(scope="module")
def data():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(140, seq_len=10, src_vocab=40, n_labels=5, seed=4, min_len=3)


@pytest.fixture(scope="module")
def oof(data):
    """Three two-epoch GRU fits by ``cross_fit``; the first member is replaced by a fit of the same fold with a fitted temperature."""
    import slnlp
    from sklearn.model_selection import StratifiedKFold
    plain = slnlp.cross_fit(make_net(data), data, cv=3, seed=41)
    train0, held0 = next(iter(StratifiedKFold(n_splits=3).split(np.zeros(len(data)), data.y)))
    assert np.array_equal(plain.folds[0], held0)
    torch.manual_seed(41)
    with_t = make_net(data, calibration={"method": "temperature"}).fit(data[train0])
    return slnlp.OutOfFold([with_t, *plain.members[1:]], plain.folds, dataset=data), plain


def _check_label_issues(est, ds, z, y, temperature=1.0, beta=1.0, **kw):
    """``est.label_issues`` against the restatement applied to the downloaded log-probs ``z`` (``beta`` / ``temperature``: those of an
    estimator that applies a temperature of its own to ``z``)."""
    from slnlp import metrics
    want = lr.audit_ref(z, y, beta=beta)
    assert lr.smallest_gap(want, y) > MARGIN
    res = est.label_issues(ds, y=y, per_row=True, **kw)
    rep = metrics.label_audit_report(lr.record_of(want), y, rank_by=kw.get("rank_by", "normalized_margin"))
    rows = res["per_row"]
    for key in ("k", "code", "flags", "pred"):
        assert np.array_equal(rows[key], want[key]), key
    assert max(_err(rows[key], want[key]) for key in ("s", "m", "other", "p_pred")) <= BOUND
    assert np.array_equal(res["joint"], want["joint"]) and res["pairs"] == [(est.classes_[g], est.classes_[c], n) for g, c, n in want["pairs"][:kw.get("pairs", 20)]]
    assert np.array_equal(np.sort(res["issues"]["row"]), np.sort(rep["issues"]["row"]))
    assert np.array_equal(res["issues"]["given"], est.classes_[y[res["issues"]["row"]]])
    assert np.array_equal(res["issues"]["suggested"], est.classes_[want["k"][res["issues"]["row"]]])
    key = rows["m"] if kw.get("rank_by", "normalized_margin") == "normalized_margin" else rows["s"]
    found = res["issues"]["row"]
    assert all((key[a], a) < (key[b], b) for a, b in zip(found[:-1], found[1:]))                # most suspicious first, ties by row
    assert abs(res["noise_rate"] - rep["noise_rate"]) <= 1e-12 and np.abs(res["per_class"]["threshold"] - want["t"])[want["n"] > 0].max() <= 2 * BOUND
    assert np.array_equal(res["per_class"]["support"], want["n"]) and res["temperature"] == temperature and res["classes"] is est.classes_
    assert (res["rows"], res["bad_labels"], res["nan_rows"]) == (len(ds), 0, 0) and res["unconfident"] == want["counts"]["unconfident"]
    assert res["argmax_disagrees"] == want["counts"]["argmax_disagrees"] and "per_row" not in est.label_issues(ds, y=y, **kw)
    return res


def test_out_of_fold_log_probs_are_each_members_own(data, oof):
    from slnlp import ops
    oof, plain = oof
    N, V = len(data), len(oof.classes_)
    assert oof.members[0].temperature_ != 1.0 and all(getattr(m, "calibration_", None) is None for m in oof.members[1:])
    z = _raw(oof, data)
    assert z.shape == (N, V) and z.dtype == np.float32 and not np.isnan(z).any()
    written = np.zeros(N, dtype=np.int64)
    for f, (m, idx) in enumerate(zip(oof.members, oof.folds)):
        own = m._forward_logp(data[idx], lambda logp, yd: logp.float())
        if f == 0:                                                               # at its temperature: scale_logp's rows
            assert z[idx].tobytes() == ops.scale_logp(own, m._cal_state).cpu().numpy().tobytes()
        else:
            assert z[idx].tobytes() == own.cpu().numpy().tobytes(), f
        written[idx] += 1
    assert (written == 1).all()                                                  # every row is written once
    import slnlp
    raw = _raw(slnlp.OutOfFold(oof.members, oof.folds, dataset=data, calibrated=False), data)
    first = oof.members[0]._forward_logp(data[oof.folds[0]], lambda logp, yd: logp.float()).cpu().numpy()
    assert raw[oof.folds[0]].tobytes() == first.tobytes() and raw[oof.folds[1]].tobytes() == z[oof.folds[1]].tobytes()
    # another data set, or these rows in another order, is refused
    for other in (data[np.arange(100)], data[np.arange(N)[::-1]]):
        with pytest.raises(ValueError, match="out-of-fold log-probs exist only for the 140 rows"):
            oof.reliability(other)
    assert np.abs(oof.predict_proba(data).sum(axis=1) - 1.0).max() <= 1e-5
    acc = float((oof.predict(data) == data.y).mean())
    print(f"out-of-fold accuracy of three 2-epoch GRU fits on {N} rows: {acc:.3f}; T of member 0 {oof.members[0].temperature_:.4f}")


def test_label_issues_and_the_other_consumers_on_out_of_fold_log_probs(data, oof):
    from confusion_ref import confusion_ref, pairs_ref
    from reliability_ref import reliability_ref, rows_ref
    oof, plain = oof
    V = len(oof.classes_)
    z = _raw(oof, data)
    y = _noisy_labels(data, V)
    res = _check_label_issues(oof, data, z, y)
    by_s = _check_label_issues(oof, data, z, y, rank_by="self_confidence", pairs=3)
    assert np.array_equal(np.sort(by_s["issues"]["row"]), np.sort(res["issues"]["row"]))
    print(f"out-of-fold audit of {len(data)} rows with 30 % of the labels redrawn: {len(res['issues']['row'])} issues, noise rate "
          f"{res['noise_rate']:.3f}, {res['unconfident']} unconfident, pairs {res['pairs'][:3]}")
    on_own = _check_label_issues(oof, data, z, np.asarray(data.y))               # the dataset's own labels
    assert on_own["argmax_disagrees"] == int((np.argmax(z, axis=1) != data.y).sum())
    # the consumers of one fit's log-probs, fed the out-of-fold ones: their own restatements on the downloaded log-probs
    rel = oof.reliability(data, y=y, bins=10)
    t = rows_ref(z, y, 10)[:, 0] * 10
    assert not np.any((np.abs(t - np.round(t)) <= 1e-6) & (np.round(t) > 0) & (np.round(t) < 10))      # no row near an inner bin edge
    ref = reliability_ref(z, y, 10)
    assert rel["temperature"] == 1.0 and (rel["rows"], rel["bad_labels"], rel["nan_rows"]) == (len(data), 0, 0)
    for k in ("ece", "mce", "brier", "nll", "accuracy", "confidence"):
        assert abs(rel[k] - ref[k]) <= BOUND * max(1.0, abs(ref[k])), (k, rel[k], ref[k])
    ea = oof.error_analysis(data, y=y, pairs=5)
    pred = np.argmax(z, axis=1)
    counts = confusion_ref(pred, y, V)
    assert np.array_equal(ea["confusion"], counts[:V * V].reshape(V, V)) and ea["accuracy"] == float((pred == y).mean())
    assert ea["pairs"] == [(int(t_), int(p_), int(c)) for t_, p_, c in pairs_ref(counts, V, 5) if c > 0]


def test_label_issues_on_a_fit_and_on_the_ensemble(data, oof):
    oof, plain = oof
    V = len(oof.classes_)
    y = _noisy_labels(data, V)
    fit = oof.members[1]
    _check_label_issues(fit, data, _raw(fit, data), y)
    hot = oof.members[0]                                                         # a fit with a temperature: at it, and at 1 when asked
    hidden = {k: hot.__dict__.pop(k) for k in ("calibration_", "temperature_") if k in hot.__dict__}
    try:
        z_hot = _raw(hot, data)
    finally:
        hot.__dict__.update(hidden)
    _check_label_issues(hot, data, z_hot, y, temperature=float(hot.temperature_), beta=hot.calibration_["beta"])
    _check_label_issues(hot, data, z_hot, y, calibrated=False)
    ens = oof.ensemble()
    assert type(ens).__name__ == "VotingEnsemble" and ens.members == oof.members
    _check_label_issues(ens, data, _raw(ens, data), y)
    with pytest.raises(ValueError, match="label_issues: 1 of 140 labels lie outside"):
        fit.label_issues(data, y=np.where(np.arange(140) == 7, V, y))


# ------------------------------------------------------------------------------------------------------------ CLI ----
def test_cli_writes_the_label_audit_with_the_key(tmp_path):
    import csv
    import json
    import os

    from slnlp import cli
    base = {"seed": 1, "cv": 2, "max_epochs": 1, "batch_size": 16, "test_size": 0.25, "scoring": ["neg_log_loss"],
            "model": "model.EncoderDecoderGRUAttn", "model_args": {"embedding_size": 16, "hidden_size": 32, "num_layers": 1, "dropout": 0.1},
            "optimizer_args": {"momentum": 0.9}, "gradient_clipping": {"gradient_clip_value": 0.5}, "grid_args": {"lr": [0.05]},
            "dataset_args": {"synthetic": {"n": 96, "seq_len": 10, "src_vocab": 40, "n_labels": 5, "seed": 4, "min_len": 3}}}
    with pytest.raises(ValueError, match="label_audit: rank_by='margin'"):       # before the grid search
        cli.run(cli.load_config(None, dict(base, workdir=str(tmp_path / "bad"), label_audit={"rank_by": "margin"})))
    assert not os.path.exists(tmp_path / "bad" / "grid_search_output.json")
    work = tmp_path / "run"
    cli.run(cli.load_config(None, dict(base, workdir=str(work), label_audit={"cv": 2, "pairs": 4, "top": 3})))
    assert {"test_output.json", "train_label_audit.json", "train_label_issues.csv"} <= set(os.listdir(work))
    got = json.load(open(work / "train_label_audit.json"))
    assert set(got) == {"rows", "bad_labels", "nan_rows", "unconfident", "argmax_disagrees", "issues", "noise_rate", "rank_by", "cv",
                        "temperature", "pairs", "per_class"}
    _, train_data = cli.load_dataset(base).split(0.25, 1)
    assert (got["rows"], got["bad_labels"], got["nan_rows"], got["rank_by"], got["cv"], got["temperature"]) == \
        (len(train_data), 0, 0, "normalized_margin", 2, 1.0)
    V = len(got["per_class"])
    assert V == len(train_data.vocab_y) and set(got["per_class"][0]) == {"class", "support", "threshold", "issues", "confident_other", "noise"}
    assert [c["support"] for c in got["per_class"]] == np.bincount(train_data.y, minlength=V).tolist()
    assert sum(c["issues"] for c in got["per_class"]) == got["issues"] and len(got["pairs"]) <= 4
    assert all(c["threshold"] is None for c in got["per_class"] if c["support"] == 0)
    lines = list(csv.reader(open(work / "train_label_issues.csv")))
    assert lines[0] == ["row", "given", "suggested", "self_confidence", "margin"] and len(lines) == 1 + min(3, got["issues"])
    for line in lines[1:]:
        assert int(line[1]) == train_data.y[int(line[0])] and int(line[2]) != int(line[1]) and 0.0 <= float(line[3]) <= 1.0
    assert [float(l[4]) for l in lines[1:]] == sorted(float(l[4]) for l in lines[1:])
