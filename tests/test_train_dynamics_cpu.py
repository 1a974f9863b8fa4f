"""CPU: the host side of ``train_dynamics`` -- the numpy restatement the GPU tests lean on (tests/train_dynamics_ref.py) on a
hand-worked example, ``metrics.train_dynamics_report``'s algebra, the margin clamps, the option's validation, the packed layout
and "off means off"."""
import math
import types

import numpy as np
import pytest

import train_dynamics_ref as R

F = 1 << 20
# rint(sigmoid(x) 2^20) of the two-column rows [x, 0] with the label in column 0: worked out by hand from sigmoid(1) = 0.7310585786,
# sigmoid(2) = 0.8807970780 (766570.48 and 923583.12 before rounding; the label in column 1 gives the complement)
Q = {1: 766570, -1: 282006, 2: 923583, -2: 124993, 0: 524288}


def z2(x):
    return [float(x), 0.0]


def hand_worked():
    """3 train rows (labels 0, 1, 0) over 4 epochs of two-column log-probs [x, 0]: row 0 is learned at epoch 2 and forgotten at
    epoch 3; row 1 is never learned; row 2 is visited twice in epoch 2 with one wrong visit, so it is not epoch-correct there (a
    forgetting event: it was right in epoch 1), and epoch 4 does not visit it at all (and visits the others in another order)."""
    y = np.array([0, 1, 0])
    epochs = [([0, 1, 2], [z2(-1), z2(1), z2(0)]),           # row 0 wrong; row 1 predicted 0: wrong; row 2 a tie: column 0 wins, right
              ([0, 1, 2, 2], [z2(1), z2(2), z2(1), z2(-1)]),
              ([0, 1, 2], [z2(-2), z2(0), z2(2)]),
              ([1, 0], [z2(1), z2(2)])]
    st = R.new_state(3)
    for e, (order, z) in enumerate(epochs, start=1):
        order = np.array(order)
        R.epoch_ref(st, np.array(z, dtype=np.float32), y[order], order, e)
    return st, y


def test_hand_worked_example_every_integer():
    st, _ = hand_worked()
    assert st["visits"].tolist() == [4, 4, 4] and st["correct_visits"].tolist() == [2, 0, 3]
    assert st["epochs_seen"].tolist() == [4, 4, 3] and st["epochs_correct"].tolist() == [2, 0, 2]
    assert st["forgetting"].tolist() == [1, 0, 1] and st["first_learned"].tolist() == [2, -1, 1] and st["last"].tolist() == [1, 0, 1]
    # row 0 sees x = -1, 1, -2, 2 under label 0; row 1 sees 1, 2, 0, 1 under label 1 (the complement); row 2 sees 0, 1, -1, 2
    q = [[Q[-1], Q[1], Q[-2], Q[2]], [Q[-1], Q[-2], Q[0], Q[-1]], [Q[0], Q[1], Q[-1], Q[2]]]
    assert st["sum_q"].tolist() == [sum(r) for r in q] == [2 * F, 1213293, 2496447]
    assert st["sum_q2"].tolist() == [sum(v * v for v in r) for r in q]
    assert st["sum_mq"].tolist() == [0, (-1 - 2 + 0 - 1) * F, (0 + 1 - 1 + 2) * F]
    assert st["head"].tolist() == [4, 12, 0, 0, 0, 3, 0, 0]


def test_hand_worked_example_every_report_field():
    from slnlp import metrics
    st, y = hand_worked()
    res = metrics.train_dynamics_report(R.record_of(st), y, rows=[10, 20, 30], top=50)
    conf = [0.5, 1213293 / (4 * F), 2496447 / (4 * F)]
    var = [math.sqrt((Q[-1] ** 2 + Q[1] ** 2 + Q[-2] ** 2 + Q[2] ** 2) / (4 * F * F) - 0.25),
           math.sqrt((2 * Q[-1] ** 2 + Q[-2] ** 2 + Q[0] ** 2) / (4 * F * F) - conf[1] ** 2),
           math.sqrt((Q[0] ** 2 + Q[1] ** 2 + Q[-1] ** 2 + Q[2] ** 2) / (4 * F * F) - conf[2] ** 2)]
    assert abs(var[0] - 0.3151) < 1e-3 and abs(var[1] - 0.1362) < 1e-3 and abs(var[2] - 0.2322) < 1e-3     # (the sizes, by hand)
    per = res["per_row"]
    assert per["row"].tolist() == [10, 20, 30] and per["label"].tolist() == [0, 1, 0] and per["visits"].tolist() == [4, 4, 4]
    assert per["confidence"].tolist() == conf and per["correctness"].tolist() == [0.5, 0.0, 0.75] and per["aum"].tolist() == [0.0, -1.0, 0.5]
    assert np.allclose(per["variability"], var, rtol=0, atol=1e-12)
    assert per["forgetting"].tolist() == [1, 0, 1] and per["first_learned"].tolist() == [2, -1, 1] and per["epochs_seen"].tolist() == [4, 4, 3]
    assert res["hard"]["row"].tolist() == [20, 10, 30] and res["hard"]["confidence"].tolist() == [conf[1], conf[0], conf[2]]
    assert res["ambiguous"]["row"].tolist() == [10, 30, 20]
    assert res["forgotten"]["row"].tolist() == [10, 30] and res["forgotten"]["forgetting"].tolist() == [1, 1]      # a tie: by row index
    assert res["low_aum"]["row"].tolist() == [20, 10, 30] and res["low_aum"]["aum"].tolist() == [-1.0, 0.0, 0.5]
    assert res["never_learned"]["row"].tolist() == [20] and res["never_learned"]["label"].tolist() == [1]
    assert res["never_learned"]["first_learned"].tolist() == [-1] and res["never_learned"]["epochs_seen"].tolist() == [4]
    for name in ("hard", "ambiguous", "forgotten", "low_aum", "never_learned"):
        assert set(res[name]) == {"row", "label", *metrics.TRAIN_DYNAMICS_FIELDS}
    assert (res["rows"], res["rows_seen"], res["unforgettable"], res["never_learned_rows"], res["forgetting_events"]) == (3, 3, 0, 1, 2)
    assert (res["epochs"], res["visits"], res["bad_labels"], res["nan_rows"], res["bad_rows"], res["overflow"]) == (4, 12, 0, 0, 0, False)
    pc = res["per_class"]
    assert pc["label"].tolist() == [0, 1] and pc["support"].tolist() == [2, 1]
    assert pc["confidence"].tolist() == [(conf[0] + conf[2]) / 2, conf[1]] and pc["correctness"].tolist() == [0.625, 0.0]
    assert pc["aum"].tolist() == [0.25, -1.0] and np.allclose(pc["variability"], [(var[0] + var[2]) / 2, var[1]], rtol=0, atol=1e-12)
    assert pc["never_learned"].tolist() == [0, 1] and pc["forgetting"].tolist() == [2, 0]


def record(visits, sum_q, sum_q2=None, sum_mq=None, correct=None, forgetting=None, first=None):
    visits = np.asarray(visits, dtype=np.int64)
    n = visits.size
    zeros = np.zeros(n, dtype=np.int64)
    return {"head": np.array([1, int(visits.sum()), 2, 3, 4, int((visits > 0).sum()), 1, 0], dtype=np.int64), "visits": visits.astype(np.int32),
            "sum_q": np.asarray(sum_q, dtype=np.int64), "sum_q2": zeros if sum_q2 is None else np.asarray(sum_q2, dtype=np.int64),
            "sum_mq": zeros if sum_mq is None else np.asarray(sum_mq, dtype=np.int64),
            "correct_visits": (zeros if correct is None else np.asarray(correct)).astype(np.int32),
            "epochs_seen": (visits > 0).astype(np.int32), "epochs_correct": zeros.astype(np.int32),
            "forgetting": (zeros if forgetting is None else np.asarray(forgetting)).astype(np.int32),
            "first_learned": (zeros - 1 if first is None else np.asarray(first)).astype(np.int32), "last": zeros.astype(np.int32)}


def test_report_algebra():
    from slnlp import metrics
    # a constant sequence has variability 0 exactly, whatever the value; confidence 1.0 is sum_q == visits 2^20
    for q in (1, 3, 282006, 766570, F - 1, F):
        for v in (1, 3, 7, 4000):
            got = metrics.train_dynamics_report(record([v], [v * q], [v * q * q]), [0])["per_row"]
            assert got["variability"][0] == 0.0 and got["confidence"][0] == q / F
    st = R.new_state(1)
    for e in range(1, 4):
        R.epoch_ref(st, np.array([[0.0, -np.inf]], dtype=np.float32), [0], None, e)
    assert st["sum_q"][0] == st["visits"][0] * F == 3 * F
    assert metrics.train_dynamics_report(R.record_of(st), [0])["per_row"]["confidence"][0] == 1.0
    # ties by row index (the dataset's, not the position's), the cut at top, unseen rows in no list, NaN means for unseen classes
    rec = record([2, 2, 0, 2, 2], [F, F, 0, F, 2 * F], [F * F // 2, F * F // 2, 0, F * F // 2, 2 * F * F], [0, 0, 0, 0, -2 * F],
                 forgetting=[1, 1, 0, 1, 0], first=[1, 1, -1, 1, -1])
    labels, rows = np.array(["b", "a", "c", "a", "b"]), [40, 30, 20, 10, 0]
    res = metrics.train_dynamics_report(rec, labels, rows=rows, top=2)
    assert res["hard"]["row"].tolist() == [10, 30]           # three rows at confidence 0.5: the first two by row index
    assert res["ambiguous"]["row"].tolist() == [0, 10]       # all four at variability 0
    assert res["forgotten"]["row"].tolist() == [10, 30] and res["low_aum"]["row"].tolist() == [0, 10]
    assert res["never_learned"]["row"].tolist() == [0]       # row 20 was never seen: in no list, though its first_learned is -1
    for name in ("hard", "ambiguous", "forgotten", "low_aum", "never_learned"):
        assert 20 not in res[name]["row"].tolist() and len(res[name]["row"]) <= 2
    full = metrics.train_dynamics_report(rec, labels, rows=rows, top=50)
    assert full["hard"]["row"].tolist() == [10, 30, 40, 0] and full["forgotten"]["row"].tolist() == [10, 30, 40]
    assert (res["rows"], res["rows_seen"], res["unforgettable"], res["never_learned_rows"], res["forgetting_events"]) == (5, 4, 0, 1, 3)
    assert (res["bad_labels"], res["nan_rows"], res["bad_rows"], res["overflow"]) == (2, 3, 4, True)
    pc = res["per_class"]
    assert pc["label"].tolist() == ["a", "b", "c"] and pc["support"].tolist() == [2, 2, 1]
    for name in ("confidence", "variability", "correctness", "aum"):
        assert np.isnan(pc[name][2]) and not np.isnan(pc[name][:2]).any(), name
        assert np.isnan(res["per_row"][name][2])
    assert pc["confidence"].tolist()[:2] == [0.5, 0.75] and pc["never_learned"].tolist() == [0, 1, 0] and pc["forgetting"].tolist() == [2, 1, 0]
    assert metrics.train_dynamics_report(rec, labels, rows=rows, top=0)["hard"]["row"].tolist() == []
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="top="):
            metrics.train_dynamics_report(rec, labels, rows=rows, top=bad)
    with pytest.raises(ValueError, match="labels has shape"):
        metrics.train_dynamics_report(rec, labels[:4], rows=rows)


def test_margin_clamps_and_codes():
    inf = np.inf
    z = np.array([[-inf, 0.0, -1.0],                          # the gold entry is -inf
                  [-inf, 0.5, -inf],                           # the gold entry is the only finite one
                  [3000.0, -3000.0, 0.0],                      # a finite margin beyond the clamp
                  [0.0, 0.0, 0.0],                             # an exact tie at the maximum: column 0 wins
                  [np.nan, 0.0, 0.0], [inf, 0.0, 0.0], [-inf, -inf, -inf], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    y = np.array([0, 1, 1, 1, 0, 0, 0, 3, -1, 0])
    order = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 10])
    vis = R.visits_ref(z, y, order, 10)
    assert vis["code"].tolist() == [0, 0, 0, 0, -2, -2, -2, -1, -1, -3]
    assert vis["mq"].tolist() == [-1024 * F, 1024 * F, -1024 * F, 0, 0, 0, 0, 0, 0, 0]
    assert vis["q"].tolist()[:2] == [0, F] and vis["q"][2] == 0 and vis["q"][3] == round(F / 3) and vis["q"].tolist()[4:] == [0] * 6
    assert vis["pred"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0] and vis["correct"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    one = R.visits_ref(np.array([[-2.5]], dtype=np.float32), [0], None, 1)                # V = 1: no other column
    assert (one["mq"][0], one["q"][0], one["correct"][0], one["code"][0]) == (0, F, 1, 0)
    assert R.visits_ref(z, y, np.full(10, -1), 10)["code"].tolist() == [-3] * 10           # the row index is looked at first
    st = R.fold(R.new_state(10), vis, 1)
    assert st["head"].tolist() == [1, 4, 2, 3, 1, 4, 0, 0] and st["visits"].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0]


def test_restatement_does_not_depend_on_the_order_of_an_epochs_visits():
    rs = np.random.RandomState(5)
    N, V, n = 7, 5, 40
    states = [R.new_state(N), R.new_state(N)]
    for e in range(1, 6):
        z = rs.randn(n, V).astype(np.float32)
        order = rs.randint(0, N - 1, size=n)                   # rows collide; row N - 1 is never seen
        y = (order * 3) % V
        z[np.arange(n), y] += np.float32(6.0) * (rs.rand(n) < 0.9)     # mostly right, so that rows are learned and forgotten again
        perm = rs.permutation(n)
        R.epoch_ref(states[0], z, y, order, e)
        R.epoch_ref(states[1], z[perm], y[perm], order[perm], e)
    for name in states[0]:
        assert np.array_equal(states[0][name], states[1][name]), name
    assert states[0]["forgetting"].sum() > 0 and states[0]["visits"][N - 1] == 0 and states[0]["last"][N - 1] == -1


def test_the_option():
    from slnlp import cli, grid
    from slnlp.net import NeuralNetClassifier
    net = NeuralNetClassifier("model.rnn.GRU")
    assert net.get_params()["train_dynamics"] is False and "train_dynamics" in NeuralNetClassifier._OWN
    on = NeuralNetClassifier(**dict(net.get_params(), train_dynamics=True))
    assert on.get_params()["train_dynamics"] is True and NeuralNetClassifier(**on.get_params()).get_params() == on.get_params()
    for bad in (1, 0, "yes", None, {"top": 5}):
        with pytest.raises(ValueError, match="train_dynamics=.*expected True or False"):
            NeuralNetClassifier("model.rnn.GRU", train_dynamics=bad).initialize()
    assert "train_dynamics" in grid.SHAPE_KEYS_EXCLUDED
    with pytest.raises(ValueError, match="train_dynamics=False"):
        net.train_dynamics()
    with pytest.raises(ValueError, match="no epoch has run"):
        on.train_dynamics()
    assert net.__dict__.get("_dyn") is None and on.__dict__.get("_dyn") is None
    # the CLI key
    assert "train_dynamics" in cli.DICT_ARGS
    assert cli.train_dynamics_options(None) is None and cli.train_dynamics_options({}) == {"top": 50}
    assert cli.train_dynamics_options({"top": 0}) == {"top": 0}
    for bad, said in ((True, "expected a dict"), ([], "expected a dict"), ({"topp": 1}, "unknown keys"), ({"top": -1}, "top=-1"),
                      ({"top": 1.5}, "top=1.5"), ({"top": True}, "top=True")):
        with pytest.raises(ValueError, match=said):
            cli.train_dynamics_options(bad)


@pytest.mark.parametrize("N", [1, 2, 5, 8])
@pytest.mark.parametrize("n_visit", [1, 3, 2049])
def test_packed_layout(N, n_visit, monkeypatch):
    import torch
    from slnlp import _lib, ops
    buf = ops.train_dynamics_buffers(N, n_visit, "cpu")
    at = buf["packed"].at
    even = lambda k: k + (k & 1)
    want = [("head", 8, 8), ("sum_q", 8, N), ("sum_q2", 8, N), ("sum_mq", 8, N)]
    want += [(name, 4, even(N)) for name in R.ROW_INTS + ("v_e", "c_e")]
    want += [("q", 8, n_visit), ("mq", 8, n_visit), ("code", 4, even(n_visit)), ("correct", 4, even(n_visit)), ("pred", 4, even(n_visit))]
    assert list(at) == [w[0] for w in want]
    off = 0
    for name, size, count in want:                           # 8-byte aligned, back to back: no piece overlaps another
        begin, dtype, shape, end, *_ = at[name]
        assert begin == off and begin % 8 == 0 and dtype.itemsize == size and end == begin + size * count, name
        assert shape == ((8,) if name == "head" else (N,) if off < at["q"][0] else (n_visit,)), name
        off = end
    assert buf["flat"].dtype == torch.int32 and buf["flat"].numel() * 4 == off and buf["shape"] == (N, n_visit)
    assert buf["state_bytes"] == at["q"][0] == 64 + 24 * N + 36 * even(N) == _lib.load().slnlp_train_dynamics_state_bytes(N)
    assert buf["sum_mq"].dtype == torch.int64 and buf["last"].shape == (N,) and buf["pred"].shape == (n_visit,)
    # what a report needs is contiguous, head through last: ONE copy, and one (longer) copy with the per-visit scratch
    buf["flat"].copy_(torch.arange(buf["flat"].numel(), dtype=torch.int32))
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append((t.numel(), t.dtype)) or real(t, *a, **k))
    got = ops.train_dynamics_download(buf)
    assert copies == [(at["last"][3] // 4, torch.int32)] and list(got) == [w[0] for w in want[:11]]
    for name in got:
        assert got[name].tobytes() == buf[name].numpy().tobytes(), name
    del copies[:]
    more = ops.train_dynamics_download(buf, per_visit=True)
    assert copies == [(buf["flat"].numel(), torch.int32)] and list(more) == [w[0] for w in want]
    assert more["pred"].tobytes() == buf["pred"].numpy().tobytes() and more["q"].dtype == np.int64
    with pytest.raises(ValueError, match="train_dynamics_buffers"):
        ops.train_dynamics_download({"flat": buf["flat"]})


def test_the_library_sizes_the_state():
    from slnlp import _lib, ops
    lib = _lib.load()
    assert lib.slnlp_train_dynamics_state_bytes(4000) == 64 + 24 * 4000 + 36 * 4000
    assert lib.slnlp_train_dynamics_state_bytes(0) == -1 and b"N=0" in lib.slnlp_last_error()
    assert lib.slnlp_train_dynamics_state_bytes(2 ** 31) == -1
    for bad in (0, -1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError, match="train_dynamics_buffers"):
            ops.train_dynamics_buffers(bad, 3, "cpu")
        with pytest.raises(ValueError, match="train_dynamics_buffers"):
            ops.train_dynamics_buffers(3, bad, "cpu")


class _Rows:
    y = np.arange(4) % 3

    def __len__(self):
        return 4


def stub_run(dyn):
    """A ``_FitRun`` with just what ``end_epoch`` reads, on the CPU: no schedule, no scoring, no valid split"""
    import torch
    from slnlp.net import _FitRun
    net = types.SimpleNamespace(history=[], lr_=0.1, verbose=0, checkpoint_dir=None, _avg_opts=None, classes_=np.arange(3))
    run = _FitRun.__new__(_FitRun)
    run.__dict__.update(net=net, schedule=None, sampler=None, balance=None, augment=None, plateau=None, es=None, wrappers=[], fast_ok=True,
                        epoch_order=None, order_dev=None, y_visit_dev=None, n_visit=4, ytr=torch.arange(4) % 3,
                        tr=_Rows(), best_valid=float("inf"), epochs_left=2, done=False,
                        t0=0.0, dynamics=dyn, _score_out={}, _rel_out={}, _rank_out={})
    return run


def test_off_means_off(monkeypatch):
    import torch
    from slnlp import ops
    calls = []
    monkeypatch.setattr(ops, "train_dynamics_epoch", lambda *a: calls.append(a))
    logp = torch.zeros(4, 3)
    run = stub_run(None)
    assert run.end_epoch((1.0, logp, [(1.0, 4)]), None) is False and run.end_epoch((1.0, logp, [(1.0, 4)]), None) is True
    assert calls == [] and len(run.net.history) == 2
    # ... and on: one call per epoch, in front of the history row, with the epoch's number, labels and order
    buf = object()
    run = stub_run({"buf": buf})
    seen = []
    monkeypatch.setattr(ops, "train_dynamics_epoch", lambda *a: seen.append(len(run.net.history)) or calls.append(a))
    run.end_epoch((1.0, logp, [(1.0, 4)]), None)
    run.order_dev = torch.tensor([3, 2, 1, 0])
    run.epoch_order, run.y_visit_dev = np.array([3, 2, 1, 0]), torch.tensor([0, 2, 1, 0])
    run.end_epoch((1.0, logp, [(1.0, 4)]), None)
    assert seen == [0, 1] and [c[3] for c in calls] == [1, 2] and all(c[0] is logp and c[4] is buf for c in calls)
    assert calls[0][2] is None and calls[0][1] is run.ytr and calls[1][2] is run.order_dev and calls[1][1] is run.y_visit_dev
