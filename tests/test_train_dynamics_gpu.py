"""GPU: training dynamics on the device -- ``slnlp_train_dynamics_reset`` / ``slnlp_train_dynamics_epoch`` through the C ABI
against the numpy restatement (tests/train_dynamics_ref.py), and ``NeuralNetClassifier(train_dynamics=True)`` on fits.

The bounds.  code, pred, correct and mq per visit are integers formed without a transcendental: they equal the restatement's.  q
is rint(p 2^20) of an fp64 probability whose ``exp`` and division may differ from numpy's by an ulp, which moves ``rint`` by at
most one unit: |q_device - q_ref| <= 1 per visit (the tests print how many visits differ at all).  Everything behind the per-visit
values is integer arithmetic: the state and the head equal the host fold of the DEVICE'S OWN per-visit values exactly, after
every one of the eight epochs of a sequence (five would not let the one-visit shape meet every kind of special visit)."""
import os

import numpy as np
import pytest
import torch

import train_dynamics_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
EPOCHS = 8                                                   # every shape meets every special visit; the fold is checked after each epoch
SPECIAL = ("nan", "label_V", "label_-1", "gold_-inf", "tie", "order_N", "order_-1", None)
# (n_visit, N, V): one wave and one thread; below a wave; V at and past a wave's 64 lanes / half of them; more rows than a block of
# 256 threads and more visits than rows' blocks; 300 visits on four rows (the atomics collide); a drop_last-style prefix
SHAPES = [(1, 1, 1), (3, 3, 3), (5, 5, 32), (8, 8, 33), (257, 255, 202), (300, 4, 65), (7, 12, 64)]
CASES = [(n, N, V, explicit) for n, N, V in SHAPES for explicit in (False, True) if explicit or n <= N]


def _right(epoch, row):
    """Whether ``row`` is to be right in ``epoch`` (1-based): always / from epoch 4 on / every other epoch / never"""
    kind = row % 4
    return kind == 0 or (kind == 1 and epoch >= 4) or (kind == 2 and epoch % 2 == 1)


def slots(n):
    """The special visits of one epoch: seven of the eight kinds where the epoch is long enough, else all visits but one (one of one)"""
    return min(7, max(1, n - 1))


def make_epoch(n, N, V, explicit, epoch, seed=0):
    """One epoch's (z float32 [n, V], y int64 [n], order int64 [n] or None).  The rows follow ``_right``'s plan, so that forgetting
    events, a late first-learned epoch and never-learned rows all occur; then the special visits: a NaN row, a label at V, a label at
    -1, a gold entry at -inf, an exact tie at the maximum (V >= 2), an order entry at N and one at -1 (with an explicit order).  An
    epoch holds ``slots(n)`` of them at distinct positions, and both the kinds and the positions rotate with the epoch, so that over
    ``EPOCHS`` epochs every shape, the one-visit shape included, meets each kind ``slots(n)`` times -- and visits without any."""
    rs = np.random.RandomState(1000 * seed + 10 * epoch + n + N + V)
    order = rs.randint(0, N, size=n) if n > N else rs.permutation(N)[:n]
    if not explicit:
        order = np.arange(n)
    y = (order * 7 + 3) % V
    z = np.round(rs.randn(n, V) * 8.0) / 4.0                 # quantised: ties happen on their own too
    for i in range(n):
        wrong = (y[i] + 1 + rs.randint(0, max(1, V - 1))) % V
        z[i, y[i] if _right(epoch, order[i]) or V == 1 else wrong] = 9.0
    z = z.astype(np.float32)
    y = y.astype(np.int64)
    order = order.astype(np.int64)
    for j in range(slots(n)):
        i, what = (j + epoch) % n, SPECIAL[(j + epoch - 1) % len(SPECIAL)]
        if what == "nan":
            z[i, rs.randint(0, V)] = np.nan
        elif what == "label_V":
            y[i] = V
        elif what == "label_-1":
            y[i] = -1
        elif what == "gold_-inf":
            z[i, y[i]] = -np.inf
        elif what == "tie" and V >= 2:
            z[i, [0, V - 1]] = 11.0
        elif what == "order_N" and explicit:
            order[i] = N
        elif what == "order_-1" and explicit:
            order[i] = -1
    return z, y, (order if explicit else None)


def _device(z, y, order, pad=3):
    """``z`` on the device, its rows V + pad floats apart (the padding is NaN: never to be read), the labels and the order."""
    n, V = z.shape
    buf = torch.full((n, V + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(z).cuda()
    return (buf[:, :V], torch.from_numpy(y).cuda(), None if order is None else torch.from_numpy(order).cuda())


def _new_buffers(N, n):
    from slnlp import ops
    buf = ops.train_dynamics_buffers(N, n, "cuda")
    buf["flat"].fill_(SENTINEL)                               # the reset, not the allocation, zeroes the state
    assert ops.train_dynamics_reset(buf) is buf
    return buf


def _state_bytes(buf):
    return buf["flat"][:buf["state_bytes"] // 4].cpu().numpy().tobytes()


_RUNS = {}


def run_sequence(case, permute=False):
    """``EPOCHS`` epochs of ``case`` through the library: (buffers, [(z, y, order, the device's per-visit download)])"""
    from slnlp import ops
    key = (case, permute)
    if key not in _RUNS:
        n, N, V, explicit = case
        buf, seen = _new_buffers(N, n), []
        for e in range(1, EPOCHS + 1):
            z, y, order = make_epoch(n, N, V, explicit, e)
            if permute:                                      # the visit positions permuted: rows, labels and order together
                perm = np.random.RandomState(e).permutation(n)
                z, y, order = z[perm], y[perm], (np.arange(n, dtype=np.int64) if order is None else order)[perm]
            zd, yd, od = _device(z, y, order)
            assert zd.stride(0) > V and ops.train_dynamics_epoch(zd, yd, od, e, buf) is buf
            seen.append((z, y, order, zd, yd, ops.train_dynamics_download(buf, per_visit=True)))
        _RUNS[key] = (buf, seen)
    return _RUNS[key]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_N%d_V%d_%s" % (c[0], c[1], c[2], "order" if c[3] else "dataset"))
def test_kernels_against_the_restatement(case):
    from slnlp import ops
    n, N, V, explicit = case
    buf, seen = run_sequence(case)
    st = R.new_state(N)
    differ = total = 0
    for e, (z, y, order, zd, yd, got) in enumerate(seen, start=1):
        want = R.visits_ref(z, y, order, N)
        for key in ("code", "correct", "pred", "mq"):
            assert np.array_equal(got[key], want[key]), (e, key, np.flatnonzero(got[key] != want[key])[:8])
        assert got["code"].dtype == got["correct"].dtype == got["pred"].dtype == np.int32 and got["mq"].dtype == got["q"].dtype == np.int64
        pred = ops.score_download(ops.score_rows(zd, yd))[0]                     # slnlp_score_rows' arg-max on the same tensors
        assert np.array_equal(got["pred"], pred)
        gap = np.abs(got["q"] - want["q"])
        assert gap.max() <= 1, (e, int(gap.max()), np.flatnonzero(gap > 1)[:8])
        differ, total = differ + int((gap > 0).sum()), total + n
        assert not got["v_e"].any() and not got["c_e"].any()                     # the fold cleared the epoch's scratch
        # the host fold of the device's own per-visit values: everything behind them is integer arithmetic
        R.fold(st, dict(got, row=want["row"]), e)
        for key in ("sum_q", "sum_q2", "sum_mq") + R.ROW_INTS:
            assert np.array_equal(got[key].astype(np.int64), st[key]), (e, key)
        assert got["head"].tolist() == st["head"].tolist(), e
    print(f"n_visit {n} N {N} V {V} {'order' if explicit else 'dataset order'}: {differ} of {total} visits differ from numpy's q by one unit; "
          f"head {st['head'].tolist()}")
    last = seen[-1][-1]
    assert last["head"][0] == EPOCHS and last["head"][6] == 0 and last["head"][7] == 0
    # every kind of special visit came slots(n) times: two kinds of bad label, the NaN row (and, with one column, the gold entry at
    # -inf, which leaves the row no finite maximum), two kinds of bad row index under an explicit order
    m = slots(n)
    assert last["head"][2:5].tolist() == [2 * m, m + (m if V == 1 else 0), 2 * m if explicit else 0]
    assert last["head"][1] == n * EPOCHS - last["head"][2:5].sum()
    if N >= 255:                                             # what the plan of the rows was made for
        seen_rows = last["visits"] > 0
        assert last["forgetting"].sum() > 0 and last["first_learned"].max() >= 4 and (last["first_learned"][seen_rows] == -1).any()
    if n < N and not explicit:
        assert (last["visits"] == 0).sum() >= N - n and (last["last"][last["visits"] == 0] == -1).all()
    if (n, N) == (300, 4):
        assert last["visits"].sum() == last["head"][1] > 4 * 60 * EPOCHS // 2     # the atomics collided, and no add was lost


@pytest.mark.parametrize("case", [(257, 255, 202, True), (300, 4, 65, True), (7, 12, 64, False)], ids=str)
def test_the_state_is_a_pure_function_of_the_arguments(case):
    buf, _ = run_sequence(case)
    want = _state_bytes(buf)
    _RUNS.pop((case, False))
    again, _ = run_sequence(case)                            # the same sequence into new buffers: the same bytes
    assert again is not buf and _state_bytes(again) == want
    moved, _ = run_sequence(case, permute=True)              # every epoch's visit positions permuted: the same state
    assert _state_bytes(moved) == want


def _raw(lib, logp, ld, y, order, n, V, N, epoch, state, state_bytes, visits, visits_bytes):
    rc = lib.slnlp_train_dynamics_epoch(logp, ld, y, order, n, V, N, epoch, state, state_bytes, visits, visits_bytes, None)
    return rc, lib.slnlp_last_error().decode()


def test_bad_arguments_return_codes_and_messages():
    from slnlp import _lib, ops
    lib = _lib.load()
    n, N, V = 6, 5, 4
    buf = _new_buffers(N, n)
    before = _state_bytes(buf)
    z = torch.zeros(n, V, device="cuda")
    y = torch.zeros(n, dtype=torch.int64, device="cuda")
    order = torch.zeros(n, dtype=torch.int64, device="cuda")
    sb = buf["state_bytes"]
    state, visits, vb = buf["flat"].data_ptr(), buf["flat"].data_ptr() + sb, buf["flat"].numel() * 4 - sb
    good = dict(logp=z.data_ptr(), ld=V, y=y.data_ptr(), order=order.data_ptr(), n=n, V=V, N=N, epoch=1, state=state, state_bytes=sb,
                visits=visits, visits_bytes=vb)
    for change, said in (({"logp": None}, "null pointer"), ({"y": None}, "null pointer"), ({"state": None}, "null pointer"),
                         ({"visits": None}, "null pointer"), ({"V": 0, "ld": 4}, "V=0 outside"), ({"n": 0}, "n_visit=0 outside"),
                         ({"N": 0}, "N=0 outside"), ({"epoch": 0}, "epoch=0 outside"), ({"epoch": -3}, "epoch=-3 outside"),
                         ({"ld": V - 1}, "ld=3 is less than V=4"), ({"state_bytes": sb - 1}, "state of %d bytes is too small" % (sb - 1)),
                         ({"visits_bytes": vb - 8}, "visits of %d bytes is too small" % (vb - 8)),
                         ({"state": state + 4}, "state is not 8-byte aligned"), ({"visits": visits + 4}, "misaligned pointer"),
                         ({"order": order.data_ptr() + 4}, "misaligned pointer"), ({"logp": z.data_ptr() + 2}, "misaligned pointer")):
        rc, msg = _raw(lib, **dict(good, **change))
        assert rc == 1 and said in msg and "train_dynamics_epoch" in msg, (change, rc, msg)
    assert lib.slnlp_train_dynamics_reset(None, sb, N, None) == 1 and b"null pointer" in lib.slnlp_last_error()
    assert lib.slnlp_train_dynamics_reset(state, sb - 8, N, None) == 1 and b"too small" in lib.slnlp_last_error()
    assert lib.slnlp_train_dynamics_reset(state + 4, sb, N, None) == 1 and b"not 8-byte aligned" in lib.slnlp_last_error()
    # the outputs overlap neither an input nor each other
    big = torch.zeros(4096, dtype=torch.int32, device="cuda")
    inside = dict(good, state=big.data_ptr(), visits=big.data_ptr() + 2048)
    for change, said in (({"logp": big.data_ptr() + 64}, "output state overlaps input logp"), ({"y": big.data_ptr() + 2048 + 16}, "output visits overlaps input y"),
                         ({"order": big.data_ptr() + sb - 8}, "output state overlaps input order"), ({"visits": big.data_ptr() + sb - 8}, "outputs state and visits overlap")):
        rc, msg = _raw(lib, **dict(inside, **change))
        assert rc == 1 and said in msg, (change, rc, msg)
    torch.cuda.synchronize()
    assert _state_bytes(buf) == before and not big.any()     # nothing was launched
    # the wrapper's own checks
    for args, said in (((z.double(), y, None, 1, buf), "logp must be"), ((z, y.int(), None, 1, buf), "y must be"), ((z, y, order[:3], 1, buf), "order must be"),
                       ((z, y, None, 0, buf), "epoch=0"), ((z[:5], y[:5], None, 1, buf), "made for 6 visits"), ((z, y, None, 1, {"flat": buf["flat"]}), "buf must be")):
        with pytest.raises(ValueError, match=said):
            ops.train_dynamics_epoch(*args)
    assert ops.train_dynamics_epoch(z, y, None, 1, buf) is buf and ops.train_dynamics_download(buf)["head"].tolist() == [1, 5, 0, 0, 1, 5, 0, 0]   # (dataset order: visit 5 is no row)


# ------------------------------------------------------------------------------------------------------ estimator ----
RNN_CFG = dict(module__embedding_size=24, module__hidden_size=32, module__num_layers=2)


def dataset(n=50, seed=6):
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(n, seq_len=12, src_vocab=64, n_labels=6, seed=seed, min_len=3)      # 40 train rows under train_split=5


def make_net(ds, seed=11, **kw):
    from slnlp.net import NeuralNetClassifier
    args = dict(module="model.EncoderDecoderGRUAttn", module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y,
                module__batch_first=True, **RNN_CFG, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1,
                optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.1, max_epochs=4, batch_size=16, device="cuda",
                gradient_clipping={"gradient_clip_value": 0.5}, train_dynamics=True)
    args.update(kw)
    net = NeuralNetClassifier(**args)
    torch.manual_seed(seed)
    return net.initialize()


@pytest.fixture
def epochs_seen(monkeypatch):
    """Every ``end_epoch`` of the test leaves {net id: [per epoch (train log-probs, labels in visit order, order or None)]}, host copies."""
    from slnlp import net as net_mod
    seen = {}
    inner = net_mod._FitRun.end_epoch

    def end_epoch(self, tr, va):
        order = self.order_dev
        seen.setdefault(id(self.net), []).append((tr[1].cpu().numpy().copy(), self.train_labels_dev().cpu().numpy().copy(),
                                                  None if order is None else order.cpu().numpy().copy()))
        return inner(self, tr, va)
    monkeypatch.setattr(net_mod._FitRun, "end_epoch", end_epoch)
    return seen


def _ref_state(got):
    """A download as the restatement's state, to go on folding from"""
    st = {name: np.asarray(got[name]).astype(np.int64).copy() for name in ("head", "sum_q", "sum_q2", "sum_mq") + R.ROW_INTS}
    return st


def _assert_state(got, st):
    """``got``, a download, against the restatement's state: exact but for q's one unit per visit"""
    for key in ("sum_mq",) + R.ROW_INTS:
        assert np.array_equal(np.asarray(got[key]).astype(np.int64), st[key]), key
    assert got["head"].tolist() == st["head"].tolist()
    v = st["visits"]
    assert (np.abs(got["sum_q"] - st["sum_q"]) <= v).all()
    assert (np.abs(got["sum_q2"] - st["sum_q2"]) <= v * (2 * R.FRAC + 1)).all()        # (q +- 1)^2 - q^2 with q <= 2^20


@pytest.mark.parametrize("mode", ["dataset_order", "shuffle", "balance", "drop_last"])
def test_the_estimator_keeps_the_restatement_of_its_own_epochs(mode, epochs_seen, monkeypatch):
    from slnlp import metrics, ops
    ds = dataset()
    net = make_net(ds, **({} if mode == "dataset_order" else {f"iterator_train__{mode}": True})).partial_fit(ds)
    recs = epochs_seen[id(net)]
    idx_tr = net._train_split(ds)[0]
    N = len(idx_tr)
    assert len(net.history) == len(recs) == 4 and N == 40
    st = R.new_state(N)
    for e, (z, y, order) in enumerate(recs, start=1):
        assert (order is None) == (mode in ("dataset_order", "drop_last")) and len(y) == z.shape[0]
        # the labels the update was given are the dataset's own labels of the rows it was given: independent of the run's accessors
        assert np.array_equal(y, ds.y[idx_tr][np.arange(len(y)) if order is None else order])
        R.epoch_ref(st, z, y, order, e)
    assert {"dataset_order": 40, "shuffle": 40, "drop_last": 32}.get(mode, recs[0][0].shape[0]) == recs[0][0].shape[0]
    _assert_state(ops.train_dynamics_download(net._dyn["buf"]), st)
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(t.numel()) or real(t, *a, **k))
    res = net.train_dynamics(top=5, per_row=True)
    assert len(copies) == 1                                  # ONE download for the report
    monkeypatch.setattr(torch.Tensor, "cpu", real)
    want = metrics.train_dynamics_report(R.record_of(st), ds.y[idx_tr], rows=idx_tr, top=5)
    per, ref = res["per_row"], want["per_row"]
    assert np.array_equal(per["row"], idx_tr) and np.array_equal(per["label"], ds.y[idx_tr])
    for key in ("visits", "forgetting", "first_learned", "epochs_seen"):
        assert np.array_equal(per[key], ref[key]), key
    seen_rows = ref["visits"] > 0
    assert np.array_equal(per["aum"][seen_rows], ref["aum"][seen_rows]) and np.array_equal(per["correctness"][seen_rows], ref["correctness"][seen_rows])
    assert np.abs(per["confidence"][seen_rows] - ref["confidence"][seen_rows]).max() <= 2.0 ** -20 + 1e-12       # one unit of q per visit
    assert np.isnan(per["confidence"][~seen_rows]).all()
    for key in ("rows", "rows_seen", "unforgettable", "never_learned_rows", "forgetting_events", "epochs", "visits", "bad_labels", "nan_rows", "bad_rows"):
        assert res[key] == want[key], key
    assert res["epochs"] == 4 and res["visits"] == sum(r[0].shape[0] for r in recs) and res["rows"] == N and not res["overflow"]
    unseen = set(idx_tr[~seen_rows].tolist())
    if mode == "drop_last":
        assert unseen == set(idx_tr[32:].tolist())
    if mode in ("dataset_order", "shuffle"):
        assert not unseen and (ref["visits"] == 4).all()
    for name in ("hard", "ambiguous", "forgotten", "low_aum", "never_learned"):
        rows = res[name]["row"].tolist()
        assert set(rows) <= set(idx_tr.tolist()) and not (set(rows) & unseen) and (name == "never_learned" or len(rows) <= 5), name
    assert res["low_aum"]["row"].tolist() == want["low_aum"]["row"].tolist() and res["forgotten"]["row"].tolist() == want["forgotten"]["row"].tolist()
    assert res["never_learned"]["row"].tolist() == want["never_learned"]["row"].tolist()
    assert "per_row" not in net.train_dynamics() and np.array_equal(res["classes"], net.classes_)
    print(f"{mode}: {res['rows_seen']} of {N} rows seen in {res['visits']} visits; {res['never_learned_rows']} never learned, "
          f"{res['forgetting_events']} forgetting events, {res['unforgettable']} unforgettable")


def test_off_allocates_and_queues_nothing(monkeypatch):
    from slnlp import ops
    calls = []
    for name in ("train_dynamics_buffers", "train_dynamics_reset", "train_dynamics_epoch"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    ds = dataset()
    net = make_net(ds, train_dynamics=False, max_epochs=1).partial_fit(ds)
    assert calls == [] and net.__dict__.get("_dyn") is None
    with pytest.raises(ValueError, match="train_dynamics=False"):
        net.train_dynamics()


def test_lockstep_fits_end_with_the_state_of_the_same_fits_alone():
    from slnlp.lockstep import fit_lockstep
    ds = dataset()
    kws = [dict(seed=11), dict(seed=12, lr=0.05)]
    alone = [make_net(ds, max_epochs=3, **kw).partial_fit(ds) for kw in kws]
    pair = [make_net(ds, max_epochs=3, **kw) for kw in kws]
    fit_lockstep(pair, [ds, ds])
    states = [_state_bytes(n._dyn["buf"]) for n in alone + pair]
    assert states[0] == states[2] and states[1] == states[3] and states[0] != states[1]
    assert pair[0].train_dynamics()["epochs"] == 3


def test_checkpoint_round_trip_and_continuation(tmp_path, epochs_seen):
    from slnlp import ops
    ds = dataset()
    net = make_net(ds, max_epochs=2).partial_fit(ds)
    net.save_params(str(tmp_path))
    assert os.path.exists(tmp_path / "train_dynamics.npz")
    saved = np.load(tmp_path / "train_dynamics.npz")
    assert np.array_equal(saved["idx_tr"], net._train_split(ds)[0]) and saved["state"].tobytes() == _state_bytes(net._dyn["buf"])
    fresh = make_net(ds, seed=5, max_epochs=2)
    fresh.load_params(str(tmp_path))
    assert _state_bytes(fresh._dyn["buf"]) == _state_bytes(net._dyn["buf"]) and fresh.train_dynamics()["epochs"] == 2
    st = _ref_state(ops.train_dynamics_download(fresh._dyn["buf"]))
    fresh.partial_fit(ds)                                    # two more epochs add to the loaded state
    recs = epochs_seen[id(fresh)]
    assert [r["epoch"] for r in fresh.history] == [1, 2, 3, 4] and len(recs) == 2
    for e, (z, y, order) in zip((3, 4), recs):
        R.epoch_ref(st, z, y, order, e)
    _assert_state(ops.train_dynamics_download(fresh._dyn["buf"]), st)
    assert st["head"][0] == 4 and (st["visits"] == 4).all()
    off = make_net(ds, train_dynamics=False)
    off.load_params(str(tmp_path))                           # the option off: the file is left alone
    assert off.__dict__.get("_dyn") is None
    other = dataset(n=60, seed=7)                            # another dataset: other train indices
    with pytest.raises(ValueError, match="train_dynamics: the state describes 40 train rows"):
        fresh.partial_fit(other)
    fresh.initialize()                                       # drops the state
    assert fresh.__dict__.get("_dyn") is None


def test_cli_writes_the_dynamics_with_the_key(tmp_path):
    import csv
    import json

    from slnlp import cli
    base = {"seed": 1, "cv": 2, "max_epochs": 3, "batch_size": 16, "test_size": 0.25, "scoring": ["neg_log_loss"],
            "model": "model.EncoderDecoderGRUAttn", "model_args": {"embedding_size": 16, "hidden_size": 32, "num_layers": 1, "dropout": 0.1},
            "optimizer_args": {"momentum": 0.9}, "gradient_clipping": {"gradient_clip_value": 0.5}, "grid_args": {"lr": [0.05]},
            "dataset_args": {"synthetic": {"n": 96, "seq_len": 10, "src_vocab": 40, "n_labels": 5, "seed": 4, "min_len": 3}}}
    with pytest.raises(ValueError, match="train_dynamics: unknown keys"):         # before the grid search
        cli.run(cli.load_config(None, dict(base, workdir=str(tmp_path / "bad"), train_dynamics={"rows": 3})))
    assert not os.path.exists(tmp_path / "bad" / "grid_search_output.json")
    work = tmp_path / "run"
    gs, _ = cli.run(cli.load_config(None, dict(base, workdir=str(work), train_dynamics={"top": 4})))
    assert {"test_output.json", "train_dynamics.json", "train_dynamics_rows.csv"} <= set(os.listdir(work))
    est = gs.best_estimator_
    res = est.train_dynamics(top=4, per_row=True)
    got = json.load(open(work / "train_dynamics.json"))
    assert set(got) == {"rows", "rows_seen", "unforgettable", "never_learned_rows", "forgetting_events", "epochs", "visits", "bad_labels", "nan_rows",
                        "bad_rows", "overflow", "top", "hard", "ambiguous", "forgotten", "low_aum", "per_class"}
    assert (got["epochs"], got["top"], got["overflow"]) == (3, 4, False) and got["rows"] == res["rows"] and got["rows_seen"] == res["rows_seen"]
    assert got["hard"] == res["hard"]["row"].tolist() and len(got["hard"]) == 4 and len(got["per_class"]) == len(res["per_class"]["label"])
    assert set(got["per_class"][0]) == {"class", "name", "support", "confidence", "variability", "correctness", "aum", "never_learned", "forgetting"}
    rows = list(csv.reader(open(work / "train_dynamics_rows.csv")))
    assert rows[0] == ["row", "label", "name", "confidence", "variability", "correctness", "forgetting", "first_learned", "aum"]
    assert len(rows) == 1 + res["rows_seen"]                 # one line per seen train row
    seen_rows = res["per_row"]["visits"] > 0
    assert [int(r[0]) for r in rows[1:]] == sorted(res["per_row"]["row"][seen_rows].tolist())
    by_row = {int(r): i for i, r in enumerate(res["per_row"]["row"])}
    for r in rows[1:]:
        i = by_row[int(r[0])]
        assert float(r[3]) == res["per_row"]["confidence"][i] and float(r[8]) == res["per_row"]["aum"][i] and int(r[6]) == res["per_row"]["forgetting"][i]
