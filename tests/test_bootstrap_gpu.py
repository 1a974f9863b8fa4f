"""GPU: the bootstrap of the scores on the device -- ``slnlp_bootstrap_scores`` through the C ABI against the numpy restatement
(tests/bootstrap_ref.py: the project's own ``metrics.scores_from_rows`` on explicitly gathered rows, itself held to sklearn on the
CPU), ``NeuralNetClassifier.score_interval`` / ``compare`` and the CLI key.

The bounds: ``counts`` are EXACTLY the restatement's, which pins the draw; ``accuracy`` and ``top_k_accuracy`` are bit-equal (an
integer over N, one division on both sides); the other count-derived columns agree to 1e-9 absolute -- the bound the project holds
the same fp64 arithmetic to elsewhere: the terms are at most 1 and there are at most 4096 of them, so the worst summation-order
error is about 1e-12 -- and the value means to 1e-9 relative to max(1, |mean|)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from bootstrap_ref import FIXED, bootstrap_ref, draws, make_case
from test_calibration_cpu import make_logp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPERATURE = {"method": "temperature"}
BOUND = 1e-9
SEED = 20261018
SHAPES = [(1, 2, 1),           # one row, one replicate
          (5, 3, 3),           # N no multiple of 4: the last Threefry call is partly used
          (257, 70, 7),        # the draws wrap the 256 threads, the classes a wave
          (1030, 300, 2),      # V > 256: the class loop strides
          (300, 202, 64),      # many classes with one row: replicates lose classes
          (64, 4096, 2)]       # V = SLNLP_CONFUSION_MAX_V: 48 KiB of class counts in LDS, the class loop strides 16 times


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(N, V, B, top_k, Q):
    """(inputs, the restatement's (stats, counts)) -- computed once, shared, never changed."""
    y, pred, rank, values = make_case(N, V, seed=N + V)
    values = values[:, :Q] if Q else None
    return (y, pred, rank, values), bootstrap_ref(y, pred, rank if top_k else None, values, V, top_k, B, SEED)


def _run(y, pred, rank, values, V, top_k, B, seed=SEED, counts=True, **kw):
    from slnlp import ops
    out = ops.bootstrap_scores(_dev(y), _dev(pred), _dev(rank), _dev(values), n_classes=V, top_k=top_k, replicates=B, seed=seed,
                               counts=counts, **kw)
    return ops.bootstrap_download(out)


def _compare(tag, got, want, top_k):
    """Hold one call to the bounds; returns (worst count-derived difference, worst relative difference of a value mean)."""
    (stats, counts), (ref_stats, ref_counts) = got, want
    assert stats.dtype == np.float64 and stats.shape == ref_stats.shape and counts.dtype == np.int32, tag
    assert np.array_equal(counts, ref_counts), tag                              # the draw, pinned
    assert stats[:, 0].tobytes() == ref_stats[:, 0].tobytes(), tag              # accuracy: integer / N on both sides
    if top_k:
        assert stats[:, 8].tobytes() == ref_stats[:, 8].tobytes(), tag
    else:
        assert np.isnan(stats[:, 8]).all(), tag
    assert np.array_equal(np.isnan(stats), np.isnan(ref_stats)), tag
    d = np.nan_to_num(np.abs(stats[:, 1:8] - ref_stats[:, 1:8])).max()
    rel = np.nan_to_num(np.abs(stats[:, FIXED:] - ref_stats[:, FIXED:]) / np.maximum(1.0, np.abs(ref_stats[:, FIXED:]))).max(initial=0.0)
    print(f"{tag}: max |device - restatement| of a score {d:.3e}, of a value mean (relative) {rel:.3e}")
    assert d <= BOUND and rel <= BOUND, tag
    return float(d), float(rel)


# ------------------------------------------------------------------------------------------------- kernels, C ABI ----
def test_the_singleton_case_loses_classes():
    """On the restatement: without this the present-class paths would go untested."""
    (y, pred, rank, values), (stats, counts) = _case(300, 202, 64, 5, 3)
    V = 202
    ts, ps = counts[:, :V], counts[:, V:2 * V]
    in_y = np.bincount(y, minlength=V) > 0
    assert ((ts[:, in_y] == 0).any(axis=1)).any(), "no replicate lacks a class of y entirely"
    assert ((ts == 0) & (ps > 0)).any(), "no replicate has a class in pred_sum only"
    assert (np.bincount(y, minlength=V) == 1).sum() >= 40, "many singleton classes"
    assert len({int(((ts[b] + ps[b]) > 0).sum()) for b in range(64)}) > 1, "the number of present classes moves"


def test_bootstrap_against_the_restatement():
    worst, worst_rel, cases = 0.0, 0.0, []
    for N, V, B in SHAPES:
        for top_k, Q in ((0, 0), (min(5, V - 1), 3)):
            inputs, want = _case(N, V, B, top_k, Q)
            y, pred, rank, values = inputs
            tag = f"N{N}_V{V}_B{B}_k{top_k}_Q{Q}"
            d, rel = _compare(tag, _run(y, pred, rank if top_k else None, values, V, top_k, B), want, top_k)
            worst, worst_rel = max(worst, d), max(worst_rel, rel)
            cases.append(tag)
    print(f"{len(cases)} calls; worst score difference {worst:.3e}, worst relative difference of a value mean {worst_rel:.3e}")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bootstrap_parity.json"), "w") as f:
        json.dump({"test": "tests/test_bootstrap_gpu.py::test_bootstrap_against_the_restatement", "device": torch.cuda.get_device_name(0),
                   "bound": BOUND, "cases": cases, "max_abs_score": worst, "max_rel_value_mean": worst_rel, "counts": "exact",
                   "accuracy_and_top_k": "bit-equal"}, f, indent=1)
        f.write("\n")


def test_values_outside_the_classes_are_never_indices():
    y, pred, rank, values = (a.copy() for a in make_case(33, 7, seed=4))
    y[3], y[20], pred[9], pred[10] = -1, 7, 11, -2
    y[14] = pred[14] = 8                                     # the same value outside the classes on both sides: no correct row
    want = bootstrap_ref(y, pred, rank, values, 7, 3, 9, SEED)
    rows = draws(33, 9, SEED)
    assert (rows == 14).any() and np.array_equal(want[0][:, 0] * 33, ((y == pred) & (y >= 0) & (y < 7))[rows].sum(axis=1))
    assert (want[1][:, -1] > 0).any() and (want[1][:, 7:14].sum(axis=1) < 33).any()          # n_bad and a skipped prediction occur
    _compare("outside", _run(y, pred, rank, values, 7, 3, 9), want, 3)
    rank[3] = 0                                              # a rank below k on a row whose label is no class: still no hit
    got = _run(y, pred, rank, values, 7, 3, 9)
    assert got[0][:, 8].tobytes() == want[0][:, 8].tobytes()


def test_values_straight_from_reliability_rows():
    from slnlp import ops
    logp, y = make_logp(257, 70, 8.0, 0.6, 1)
    z, yd = torch.from_numpy(logp).cuda(), torch.from_numpy(y).cuda()
    pred, _, rank, _ = ops.score_rows(z, yd)
    rows, _ = ops.reliability_rows(z, yd)
    assert rows[:, :3].stride() == (4, 1)                    # ldv = 4, Q = 3: conf, brier, nll
    got = ops.bootstrap_download(ops.bootstrap_scores(yd, pred, rank, rows[:, :3], n_classes=70, top_k=5, replicates=7, seed=SEED, counts=True))
    want = bootstrap_ref(y, pred.cpu().numpy(), rank.cpu().numpy(), rows.cpu().numpy()[:, :3], 70, 5, 7, SEED)
    _compare("reliability_rows", got, want, 5)


def test_padding_is_not_read_and_a_nan_row_propagates():
    y, pred, rank, values = make_case(257, 70, seed=9)
    padded = torch.full((257, 5), float("nan"), dtype=torch.float64, device="cuda")
    padded[:, :3] = torch.from_numpy(values).cuda()
    want = bootstrap_ref(y, pred, rank, values, 70, 5, 7, SEED)
    from slnlp import ops
    got = ops.bootstrap_download(ops.bootstrap_scores(_dev(y), _dev(pred), _dev(rank), padded[:, :3], n_classes=70, top_k=5, replicates=7,
                                                      seed=SEED, counts=True))
    assert not np.isnan(got[0]).any()
    _compare("padded", got, want, 5)
    holed = values.copy()
    holed[100, 1] = np.nan
    want = bootstrap_ref(y, pred, rank, holed, 70, 5, 7, SEED)
    drawn = (draws(257, 7, SEED) == 100).any(axis=1)
    assert drawn.any() and not drawn.all()                   # on the restatement: some replicates hold the row, some do not
    got = _run(y, pred, rank, holed, 70, 5, 7)
    assert np.array_equal(np.isnan(got[0][:, FIXED + 1]), drawn) and not np.isnan(np.delete(got[0], FIXED + 1, axis=1)).any()
    _compare("nan_row", got, want, 5)


def test_the_result_is_a_pure_function_of_the_arguments():
    from slnlp import ops
    (y, pred, rank, values), want = _case(257, 70, 7, 5, 3)
    args = (_dev(y), _dev(pred), _dev(rank), _dev(values))
    kw = dict(n_classes=70, top_k=5, seed=SEED, counts=True)
    out = ops.bootstrap_scores(*args, replicates=7, **kw)
    assert out[0].untyped_storage().data_ptr() == out[1].untyped_storage().data_ptr()       # slices of one allocation
    stats, counts = ops.bootstrap_download(out)
    first = stats.tobytes() + counts.tobytes()
    again = ops.bootstrap_download(ops.bootstrap_scores(*args, replicates=7, out=out, **kw))          # over its own leftovers
    assert again[0].tobytes() + again[1].tobytes() == first
    other = (torch.full((7, 12), float("nan"), dtype=torch.float64, device="cuda"), torch.full((7, 211), -7, dtype=torch.int32, device="cuda"))
    again = ops.bootstrap_download(ops.bootstrap_scores(*args, replicates=7, out=other, **kw))
    assert again[0].tobytes() + again[1].tobytes() == first
    # replicate b does not depend on B
    three = ops.bootstrap_download(ops.bootstrap_scores(*args, replicates=3, **kw))
    assert three[0].tobytes() == stats[:3].tobytes() and three[1].tobytes() == counts[:3].tobytes()
    # another seed draws other rows
    moved = ops.bootstrap_download(ops.bootstrap_scores(*args, replicates=7, **dict(kw, seed=SEED + 1)))
    assert not np.array_equal(moved[1], counts)
    assert np.array_equal(moved[1], bootstrap_ref(y, pred, rank, values, 70, 5, 7, SEED + 1)[1])
    big = ops.bootstrap_download(ops.bootstrap_scores(*args, replicates=2, **dict(kw, seed=2 ** 64 - 1)))      # the key's high word
    assert np.array_equal(big[1], bootstrap_ref(y, pred, rank, values, 70, 5, 2, 2 ** 64 - 1)[1])
    # the pairing: another fit's predictions under the same seed meet the same resamples
    rival = np.random.RandomState(1).randint(0, 70, size=257).astype(np.int32)
    paired = ops.bootstrap_download(ops.bootstrap_scores(args[0], _dev(rival), args[2], args[3], replicates=7, **kw))
    assert np.array_equal(paired[1][:, :70], counts[:, :70]) and not np.array_equal(paired[1][:, 70:140], counts[:, 70:140])
    assert paired[0][:, FIXED:].tobytes() == stats[:, FIXED:].tobytes()
    # without counts: the same stats, one tensor
    lean = ops.bootstrap_scores(*args, replicates=7, **dict(kw, counts=False))
    assert lean[1] is None and ops.bootstrap_download(lean)[0].tobytes() == stats.tobytes()


def test_the_download_is_one_copy(monkeypatch):
    from slnlp import ops
    (y, pred, rank, values), _ = _case(257, 70, 7, 5, 3)
    out = ops.bootstrap_scores(_dev(y), _dev(pred), _dev(rank), _dev(values), n_classes=70, top_k=5, replicates=7, seed=SEED, counts=True)
    z, yd = torch.from_numpy(make_logp(257, 70, 8.0, 0.6, 1)[0]).cuda(), _dev(y)
    buf = ops.score_interval_rows(z, yd, ops.score_interval_buffers(257, 70, 7, "cuda"), top_k=5, seed=SEED)
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(t.numel()) or real(t, *a, **k))
    ops.bootstrap_download(out)
    got = ops.score_interval_download(buf)
    monkeypatch.undo()
    assert copies == [7 * 12 + (7 * 211 + 1) // 2, buf["head"]] and buf["head"] < buf["flat"].numel() - 4 * 257 + 4      # the rows stay
    pred, _, rank, counts = ops.score_download(ops.score_rows(z, yd))
    assert np.array_equal(got["pred"], pred) and np.array_equal(got["rank"], rank) and np.array_equal(got["counts"], counts)
    rows, table = ops.reliability_rows(z, yd)
    assert got["table"].tobytes() == table.cpu().numpy().tobytes()
    want = bootstrap_ref(y, pred, rank, rows.cpu().numpy()[:, :3], 70, 5, 7, SEED)
    _compare("pipeline", (got["stats"], want[1].astype(np.int32)), want, 5)


def test_bad_arguments_return_codes_and_messages():
    from slnlp import _lib, ops
    lib = _lib.load()
    y, pred, rank, values = (_dev(a) for a in make_case(5, 3, seed=1))
    values = torch.cat([values, values[:, :1]], dim=1).contiguous()                     # [5, 4]: ldv = 4
    stats = torch.full((4 * 12 + 16,), 7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((4 * 10 + 16,), 9, dtype=torch.int32, device="cuda")
    p, st = _lib.ptr, _lib.stream_ptr()
    good = (p(y), p(pred), p(rank), p(values), 4, 3, 5, 3, 2, 4, 7, p(stats), p(counts))
    cases = [(0, None, "null pointer"), (1, None, "null pointer"), (2, None, "null pointer"), (3, None, "null pointer"),
             (11, None, "null pointer"), (6, 0, "N=0 outside"), (6, 2 ** 31, "N=2147483648"), (7, 0, "V=0 outside 1..4096"),
             (7, 4097, "V=4097 outside 1..4096"), (9, 0, "B=0 outside 1..65536"), (9, 65537, "B=65537"), (5, -1, "Q=-1 outside 0..8"),
             (5, 9, "Q=9 outside 0..8"), (4, 2, "ldv=2 is less than Q=3"), (4, 2 ** 62, "is no addressable matrix"), (8, -1, "top_k=-1"),
             (8, 3, "top_k=3 outside [1, 3)"), (0, p(y) + 4, "misaligned"), (1, p(pred) + 2, "misaligned"), (2, p(rank) + 2, "misaligned"),
             (3, p(values) + 4, "misaligned"), (11, p(stats) + 4, "misaligned"), (12, p(counts) + 2, "misaligned"),
             (11, p(values), "output stats overlaps input values"), (11, p(y), "output stats overlaps input y"),
             (12, p(pred), "output counts overlaps input pred"), (12, p(rank), "output counts overlaps input rank"),
             (12, p(stats) + 8, "stats and counts overlap")]
    for i, value, text in cases:
        args = list(good)
        args[i] = value
        rc, msg = lib.slnlp_bootstrap_scores(*args, st), lib.slnlp_last_error().decode()
        assert rc == 1 and "bootstrap_scores" in msg and text in msg, (i, value, rc, msg)
    torch.cuda.synchronize()                                                    # no sticky error: nothing faulted ...
    assert bool((stats == 7.0).all()) and bool((counts == 9).all())             # ... and nothing was launched
    # the nullable ones: rank with top_k = 0, values with Q = 0, counts
    assert lib.slnlp_bootstrap_scores(p(y), p(pred), None, None, 0, 0, 5, 3, 0, 4, 7, p(stats), None, st) == 0
    torch.cuda.synchronize()
    assert bool((stats[:36] != 7.0).all()) and bool((stats[36:] == 7.0).all()) and bool((counts == 9).all())
    assert lib.slnlp_abi_version() == 1
    for kw in ({"replicates": 0}, {"replicates": 65537}, {"replicates": 2.5}, {"seed": -1}, {"seed": 2 ** 64}, {"top_k": 3}, {"top_k": -1},
               {"n_classes": 0}, {"n_classes": 4097}):
        with pytest.raises(ValueError, match="bootstrap_scores: (replicates|seed|top_k|n_classes)="):
            ops.bootstrap_scores(y, pred, rank, **dict(dict(n_classes=3, replicates=4, seed=0), **kw))
    for bad in ((y.int(), pred, rank, None), (y, pred.long(), rank, None), (y, pred, None, None), (y, pred, rank[:4], None),
                (y, pred, rank, values.float()), (y, pred, rank, values[:4]), (y, pred, rank, values[:, ::2])):
        with pytest.raises(ValueError, match="bootstrap_scores"):
            ops.bootstrap_scores(*bad, n_classes=3, top_k=2, replicates=4, seed=0)
    with pytest.raises(ValueError, match="bootstrap_scores: out"):
        ops.bootstrap_scores(y, pred, rank, n_classes=3, top_k=2, replicates=4, seed=0, out=(stats[:36].view(4, 9), counts[:39].view(3, 13)))


# ------------------------------------------------------------------------------------------------------ estimator ----
from test_calibration_gpu import RNN_CFG, _same, _sd, _strip, make_net, raw_logp  # noqa: E402

META = ("replicates", "level", "seed", "rows")


@pytest.fixture(scope="module")
def ds():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(120, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


@pytest.fixture(scope="module")
def calibrated(ds):
    return make_net(ds, calibration=TEMPERATURE).partial_fit(ds)


def _noisy_labels(data, V):
    """The dataset's labels with three in ten redrawn: a tiny fit is right on every row of the data it saw, which would leave
    nothing to resample."""
    rs = np.random.RandomState(0)
    y = np.asarray(data.y, dtype=np.int64)
    return np.where(rs.rand(len(y)) < 0.3, rs.randint(0, V, size=len(y)), y)


def _check_interval(net, data, y=None, **kw):
    """``net.score_interval`` against the existing scoring paths and the restatement (``y``: labels apart from the dataset's)."""
    from slnlp import metrics
    res = net.score_interval(data, y=y, replicates=200, seed=3, return_replicates=True, **kw)
    names = res["names"]
    assert names == [*metrics.BOOT_COLUMNS, "confidence", "neg_brier", "neg_log_loss"]
    assert set(res) == set(names) | set(META) | {"names", "replicate_scores"}
    assert (res["replicates"], res["level"], res["seed"], res["rows"]) == (200, 0.95, 3, len(data))
    # the points: the existing host scoring on the log-probs predict_proba starts from, and the reliability table
    z = torch.from_numpy(raw_logp(net, data))
    y = np.asarray(data.y if y is None else y, dtype=np.int64)
    pred, picked, rank, counts = metrics.reduce_rows(z, torch.from_numpy(y))
    want = metrics.scores_from_rows(list(metrics.BOOT_COLUMNS), y, pred, picked, rank, counts, z.shape[1])
    rel = net.reliability(data, y=y, **kw)
    want.update(confidence=rel["confidence"], neg_brier=-rel["brier"], neg_log_loss=-rel["nll"])
    reps = res["replicate_scores"]
    assert reps.shape == (200, len(names)) and reps.dtype == np.float64
    for i, name in enumerate(names):
        r = res[name]
        assert set(r) == {"point", "mean", "std", "lower", "upper", "n_nan"} and r["n_nan"] == 0, name
        assert r["point"] == want[name], (name, r["point"], want[name])
        assert r["lower"] <= r["mean"] <= r["upper"] and r["std"] >= 0.0, (name, r)
        alpha = 1.0 - 0.95
        lower, upper = np.quantile(reps[:, i], [alpha / 2, 1 - alpha / 2])
        assert (r["lower"], r["upper"], r["mean"]) == (lower, upper, np.ascontiguousarray(reps[:, i]).mean()), name
    assert res["accuracy"]["point"] == float((z.argmax(1).numpy() == y).mean()) and res["accuracy"]["std"] > 0.0
    # the replicates are the restatement's on the downloaded per-row results
    ref = bootstrap_ref(y, pred, rank, None, z.shape[1], 2, 200, 3)[0]
    assert reps[:, 0].tobytes() == ref[:, 0].tobytes() and reps[:, 8].tobytes() == ref[:, 8].tobytes()
    assert np.abs(reps[:, 1:8] - ref[:, 1:8]).max() <= BOUND
    return res


def _plain(res):
    return json.dumps({k: v for k, v in res.items() if k not in ("replicate_scores",)}, sort_keys=True)


def test_score_interval_of_a_calibrated_fit(ds, calibrated, monkeypatch):
    net = calibrated
    assert net.temperature_ != 1.0
    before, hist = _sd(net), _strip(net.history)
    noisy = _noisy_labels(ds, len(net.classes_))
    on = _check_interval(net, ds, y=noisy)
    off = _check_interval(net, ds, y=noisy, calibrated=False)
    assert (on["neg_brier"]["lower"], on["neg_brier"]["upper"]) != (off["neg_brier"]["lower"], off["neg_brier"]["upper"])
    assert on["neg_log_loss"]["point"] != off["neg_log_loss"]["point"]
    assert all(on[n] == off[n] for n in on["names"][:9])                          # the arg-max never moves
    # the same seed gives the same dict, another seed another one; ONE download per call
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(t.numel()) or real(t, *a, **k))
    again = net.score_interval(ds, y=noisy, replicates=200, seed=3)
    monkeypatch.undo()
    assert len(copies) == 1, copies
    assert _plain(again) == _plain({k: v for k, v in on.items() if k != "names"})
    assert _plain(net.score_interval(ds, y=noisy, replicates=200, seed=4)) != _plain(again)
    # a subset of names, another k, another level
    some = net.score_interval(ds, y=noisy, scoring=["top3_accuracy", "f1_macro", "neg_brier"], replicates=200, seed=3, level=0.5)
    assert set(some) == {"top3_accuracy", "f1_macro", "neg_brier", *META} and some["level"] == 0.5
    assert some["f1_macro"]["point"] == on["f1_macro"]["point"] and some["f1_macro"]["mean"] == on["f1_macro"]["mean"]
    assert on["f1_macro"]["lower"] <= some["f1_macro"]["lower"] <= some["f1_macro"]["upper"] <= on["f1_macro"]["upper"]
    assert some["f1_macro"]["upper"] - some["f1_macro"]["lower"] < on["f1_macro"]["upper"] - on["f1_macro"]["lower"]
    assert some["top3_accuracy"]["point"] >= on["top_k_accuracy"]["point"]
    assert net.score_interval(ds, y=noisy, scoring="accuracy", replicates=7)["accuracy"]["point"] == on["accuracy"]["point"]
    assert net.score_interval(ds, scoring="accuracy", replicates=7)["accuracy"]["point"] == float((net.predict(ds) == ds.y).mean())     # the dataset's own labels
    # a fit against itself: no difference in any replicate
    same = net.compare(net, ds, y=noisy, replicates=50, seed=1, return_replicates=True)
    assert set(same) == set(on) and not same["replicate_scores"].any()
    for name in same["names"]:
        assert same[name] == {"point": 0.0, "mean": 0.0, "std": 0.0, "lower": 0.0, "upper": 0.0, "n_nan": 0, "p_not_better": 1.0}, name
    # nothing leaves a trace
    assert _same(_sd(net), before) and _strip(net.history) == hist
    # what is rejected
    wrong = np.asarray(ds.y).copy()
    wrong[3] = len(net.classes_)
    with pytest.raises(ValueError, match=f"score_interval: 1 of 120 labels lie outside the {len(net.classes_)} classes of the log-probs"):
        net.score_interval(ds, y=wrong, replicates=5)
    with pytest.raises(ValueError, match="shape"):
        net.score_interval(ds, y=wrong[:5])
    with pytest.raises(ValueError, match="neg_ece has no bootstrap interval"):
        net.score_interval(ds, scoring=["accuracy", "neg_ece"])


def test_compare_a_gru_fit_with_a_transformer_fit(ds, calibrated):
    from slnlp.net import NeuralNetClassifier
    gru = make_net(ds, module="model.EncoderDecoderGRUAttn", cfg=RNN_CFG).partial_fit(ds)
    b = _check_interval(gru, ds)
    a = calibrated.score_interval(ds, replicates=200, seed=3, return_replicates=True)
    diff = calibrated.compare(gru, ds, replicates=200, seed=3, return_replicates=True)
    assert diff["replicate_scores"].tobytes() == (a["replicate_scores"] - b["replicate_scores"]).tobytes()       # one seed, the same rows
    for i, name in enumerate(diff["names"]):
        d = diff[name]
        assert d["point"] == a[name]["point"] - b[name]["point"] and 0.0 <= d["p_not_better"] <= 1.0, name
        assert d["lower"] <= d["mean"] <= d["upper"], name
        assert d["p_not_better"] == float(np.mean(diff["replicate_scores"][:, i] <= 0.0)), name
    back = gru.compare(calibrated, ds, replicates=200, seed=3)
    assert back["accuracy"]["mean"] == -diff["accuracy"]["mean"] and abs(back["accuracy"]["lower"] + diff["accuracy"]["upper"]) <= 1e-12
    stranger = NeuralNetClassifier(module="model.Transformer")
    stranger.initialized_, stranger.classes_ = True, np.arange(len(gru.classes_) + 1)
    with pytest.raises(ValueError, match="compare: the two fits have different classes_"):
        gru.compare(stranger, ds)


# ------------------------------------------------------------------------------------------------------------ CLI ----
def test_cli_writes_the_intervals_with_the_key(tmp_path):
    from slnlp import cli
    base = {"seed": 1, "cv": 2, "max_epochs": 2, "batch_size": 16, "test_size": 0.25,
            "scoring": ["neg_log_loss", "f1_macro", "top3_accuracy", "neg_ece"],
            "model": "model.Transformer", "model_args": {"embedding_size": 16, "hidden_size": 32, "num_layers": 1, "dropout": 0.1, "num_heads": 2},
            "optimizer_args": {"momentum": 0.9}, "gradient_clipping": {"gradient_clip_value": 0.5}, "grid_args": {"lr": [0.05]},
            "dataset_args": {"synthetic": {"n": 96, "seq_len": 10, "src_vocab": 40, "n_labels": 5, "seed": 4, "min_len": 3}}}
    work = tmp_path / "run"
    gs, test_output = cli.run(cli.load_config(None, dict(base, workdir=str(work), confidence_intervals={"replicates": 100, "seed": 5})))
    assert {"test_output.json", "test_intervals.json"} <= set(os.listdir(work))
    got = json.load(open(work / "test_intervals.json"))
    test_data, _ = cli.load_dataset(base).split(0.25, 1)
    assert (got["replicates"], got["level"], got["seed"], got["rows"]) == (100, 0.95, 5, len(test_data))
    named = ["accuracy", "neg_log_loss", "f1_macro", "top3_accuracy"]             # every name of the run but the one without an interval
    assert sorted(got["intervals"]) == sorted(f"test_{n}" for n in named)
    want = gs.best_estimator_.score_interval(test_data, scoring=named, replicates=100, seed=5)
    for n in named:
        assert got["intervals"][f"test_{n}"] == want[n], n
        assert got["intervals"][f"test_{n}"]["lower"] <= got["intervals"][f"test_{n}"]["upper"]
    for n in ("accuracy", "f1_macro", "top3_accuracy"):                          # the same numbers test_output.json holds
        assert got["intervals"][f"test_{n}"]["point"] == pytest.approx(test_output[f"test_{n}"], abs=1e-12), n
