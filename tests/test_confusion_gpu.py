"""GPU: error analysis on the device -- ``slnlp_topk_rows``, ``slnlp_confusion_matrix`` and ``slnlp_confusion_pairs`` through the C
ABI against the numpy restatement (tests/confusion_ref.py, itself held to sklearn and a direct fp64 softmax on the CPU),
``NeuralNetClassifier.predict_topk`` / ``error_analysis`` and the CLI key.

The bounds: the top-k indices, the matrix and the pairs are EXACTLY the restatement's; the probabilities agree to 1e-9 absolute --
the bound tests/test_reliability_gpu.py holds the same fp64 arithmetic to -- and their first column is ``reliability_rows``' conf
bit for bit."""
import csv
import json
import os

import numpy as np
import pytest
import torch

from confusion_ref import class_report_ref, confusion_ref, handmade_rows, pairs_ref, topk_ref
from test_calibration_cpu import make_logp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPERATURE = {"method": "temperature"}
BOUND = 1e-9
BETAS = (None, 0.16, 6.25)
PAIR_CASES = [(2000, 12, 0.3, 0.2, 1), (300, 202, 3.0, 0.5, 2), (5, 3, 2.0, 0.6, 1)]


def _device(logp, y, ld=None):
    """``logp`` on the device, its rows ``ld`` floats apart (the padding is NaN: never to be read), and the labels."""
    N, V = logp.shape
    buf = torch.full((N, ld or V), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(logp).cuda()
    return buf[:, :V], torch.from_numpy(np.asarray(y, dtype=np.int64)).cuda()


def _kernel_cases():
    cases = [("N1_V2", np.log(np.array([[0.83, 0.17]], dtype=np.float32)), np.array([1]), None),
             ("N5_V3", *make_logp(5, 3, 2.0, 0.6, 1), None),
             ("N257_V70", *make_logp(257, 70, 8.0, 0.6, 1), None),              # rows wrap a block's four waves, columns the 64 lanes
             ("N33_V129_ld136", *make_logp(33, 129, 4.0, 0.6, 3), 136),
             ("N300_V202_ties", *make_logp(300, 202, 0.3, 0.2, 7), None)]        # three rows hold tied float32 values
    return cases + [(name, logp, y if len(y) == len(logp) else np.zeros(len(logp), dtype=np.int64), None)
                    for name, (logp, y) in handmade_rows().items()]


def _ks(V):
    return sorted({k for k in (1, 2, 5, min(V, 64)) if k <= V})


def _bytes(*tensors):
    return b"".join(t.cpu().numpy().tobytes() for t in tensors)


# ------------------------------------------------------------------------------------------------- kernels, C ABI ----
def test_topk_against_the_restatement():
    from slnlp import ops
    worst, calls = 0.0, 0
    for name, logp, y, ld in _kernel_cases():
        z, yd = _device(logp, y, ld)
        pred = ops.score_rows(z, yd)[0].cpu().numpy()
        for beta in BETAS:
            state = None if beta is None else ops.temperature_state(beta, "cuda")
            conf = ops.reliability_rows(z, yd, state=state)[0][:, 0].cpu().numpy()
            for k in _ks(logp.shape[1]):
                idx, prob = ops.topk_download(ops.topk_rows(z, k, state=state))
                want_idx, want_prob = topk_ref(logp, k, 1.0 if beta is None else beta)
                tag = (name, beta, k)
                assert idx.dtype == np.int32 and prob.dtype == np.float64 and idx.shape == prob.shape == (len(y), k), tag
                assert np.array_equal(idx, want_idx), tag
                assert np.array_equal(idx[:, 0], pred), tag
                assert np.array_equal(np.isnan(prob), np.isnan(want_prob)), tag
                d = np.abs(prob - want_prob)[~np.isnan(want_prob)]
                print(f"{tag}: max |device - restatement| = {d.max(initial=0.0):.3e}")
                assert d.max(initial=0.0) <= BOUND, tag
                assert prob[:, 0].tobytes() == conf.tobytes(), tag                  # reliability_rows' conf, bit for bit
                worst, calls = max(worst, float(d.max(initial=0.0))), calls + 1
        if ld is not None:
            assert bool(torch.isnan(z._base[:, logp.shape[1]:]).all())
    print(f"{calls} calls; max |device - restatement| of a probability: {worst:.3e}")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "confusion_parity.json"), "w") as f:
        json.dump({"test": "tests/test_confusion_gpu.py::test_topk_against_the_restatement", "device": torch.cuda.get_device_name(0),
                   "bound": BOUND, "calls": calls, "max_abs_prob": worst, "cases": [c[0] for c in _kernel_cases()],
                   "k": "1, 2, 5, min(V, 64)", "beta": list(BETAS), "indices": "exact", "first_column": "reliability_rows' conf, bit for bit"},
                  f, indent=1)
        f.write("\n")


def _scored(logp, y, ld=None):
    from slnlp import ops
    z, yd = _device(logp, y, ld)
    pred, _, _, counts = ops.score_rows(z, yd)
    return pred, yd, counts.cpu().numpy().astype(np.int64)


def test_matrix_is_exact():
    from slnlp import ops
    for name, logp, y, ld in _kernel_cases() + [("N2000_V12", *make_logp(2000, 12, 0.3, 0.2, 1), None)]:
        V = logp.shape[1]
        pred, yd, score = _scored(logp, y, ld)
        counts = ops.confusion_matrix(pred, yd, V).cpu().numpy()
        assert counts.dtype == np.int32 and np.array_equal(counts, confusion_ref(pred.cpu().numpy(), y, V)), name
        C = counts[:V * V].reshape(V, V)
        assert counts[V * V] == 0 and C.sum() == len(y), name
        assert np.array_equal(C.sum(axis=1), score[:V]) and np.array_equal(np.diag(C), score[2 * V:3 * V]), name
        assert np.array_equal(C.sum(axis=0), score[V:2 * V]), name


def test_matrix_counts_what_is_no_class_in_the_tail():
    from slnlp import ops
    logp, y = make_logp(33, 7, 2.0, 0.6, 4)
    y[3], y[20] = -1, 7
    pred, yd, score = _scored(logp, y)
    C = ops.confusion_matrix(pred, yd, 7).cpu().numpy()
    assert C[49] == 2 == score[21] and np.array_equal(C, confusion_ref(pred.cpu().numpy(), y, 7))
    assert np.array_equal(C[:49].reshape(7, 7).sum(axis=1), score[:7]) and np.array_equal(np.diag(C[:49].reshape(7, 7)), score[14:21])
    wild = pred.clone()
    wild[9], wild[10] = 7, -1                               # no prediction of score_rows': the call still never indexes with it
    C = ops.confusion_matrix(wild, yd, 7).cpu().numpy()
    assert C[49] == 4 and np.array_equal(C, confusion_ref(wild.cpu().numpy(), y, 7)) and C.sum() == 33


@pytest.mark.parametrize("case", PAIR_CASES)
def test_pairs_are_exact(case):
    from slnlp import _lib, ops
    logp, y = make_logp(*case)
    V = logp.shape[1]
    pred, yd, _ = _scored(logp, y)
    counts = ops.confusion_matrix(pred, yd, V)
    ref_counts = confusion_ref(logp.argmax(axis=1), y, V)
    assert np.array_equal(counts.cpu().numpy(), ref_counts)
    for M in (1, 20, 64):
        want = pairs_ref(ref_counts, V, M)
        got = ops.confusion_pairs(counts, V, M)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (case, M)
        # purity: over its own leftovers, into foreign buffers with a larger, dirty workspace, the matrix without its tail entry
        assert _bytes(ops.confusion_pairs(counts, V, M, out=got)) == want.tobytes()
        need = _lib.load().slnlp_confusion_pairs_workspace_bytes(V, M)
        other = torch.full((M, 3), 77, dtype=torch.int32, device="cuda")
        ops.confusion_pairs(counts[:V * V], V, M, out=other, work=torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device="cuda"))
        assert _bytes(other) == want.tobytes(), (case, M)
    if V == 3:
        assert want[4:].tolist() == [[-1, -1, 0]] * 60 and (want[:4, 2] > 0).all()


def test_the_results_are_pure_functions_of_the_arguments():
    from slnlp import ops
    logp, y = make_logp(300, 202, 0.3, 0.2, 7)
    z, yd = _device(logp, y)
    state = ops.temperature_state(0.16, "cuda")
    out = ops.topk_buffers(300, 5, "cuda")
    assert out[0].untyped_storage().data_ptr() == out[1].untyped_storage().data_ptr()       # slices of one allocation
    assert ops.topk_rows(z, 5, state=state, out=out) is out
    a = _bytes(*out)
    assert _bytes(*ops.topk_rows(z, 5, state=state, out=out)) == a                          # over its own leftovers
    other = (torch.full((300, 5), -7, dtype=torch.int32, device="cuda"), torch.full((300, 5), float("nan"), dtype=torch.float64, device="cuda"))
    assert _bytes(*ops.topk_rows(z, 5, state=state, out=other)) == a
    assert _bytes(*ops.topk_rows(z, 5, state=state)) == a
    one = _bytes(*ops.topk_rows(z, 5, state=ops.temperature_state(1.0, "cuda")))          # beta = 1 from a state and as the null pointer
    assert one == _bytes(*ops.topk_rows(z, 5)) != a
    pred = ops.score_rows(z, yd)[0]
    first = ops.confusion_matrix(pred, yd, 202)
    b = _bytes(first)
    assert _bytes(ops.confusion_matrix(pred, yd, 202, out=first)) == b
    assert _bytes(ops.confusion_matrix(pred, yd, 202, out=torch.full((202 * 202 + 1,), 9, dtype=torch.int32, device="cuda"))) == b


def test_downloads_are_one_copy(monkeypatch):
    from slnlp import ops
    logp, y = make_logp(257, 70, 8.0, 0.6, 1)
    z, yd = _device(logp, y)
    buf = ops.error_analysis_rows(z, yd, ops.error_analysis_buffers(257, 70, 5, 20, "cuda"))
    top = ops.topk_rows(z, 5)
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(t.numel()) or real(t, *a, **k))
    small = ops.error_analysis_download(buf, matrix=False, topk=False)
    mid = ops.error_analysis_download(buf, matrix=False, topk=True)
    full = ops.error_analysis_download(buf, matrix=True, topk=True)
    idx, prob = ops.topk_download(top)
    monkeypatch.undo()
    # the pairs and the class counts; one pad entry at most in front of the lists; the matrix only when asked for
    assert copies[0] == 60 + 211 and copies[1] - copies[0] - 3 * 257 * 5 in (0, 1) and copies[2] == copies[1] + 4901 and copies[3] == 3 * 257 * 5
    assert small["confusion"] is None and small["topk_idx"] is None and mid["confusion"] is None
    want_idx, want_prob = topk_ref(logp, 5)
    for got in (mid, full):
        assert np.array_equal(got["topk_idx"], want_idx) and np.array_equal(got["topk_idx"], idx) and got["topk_prob"].tobytes() == prob.tobytes()
        assert np.abs(got["topk_prob"] - want_prob).max() <= BOUND
    ref = confusion_ref(logp.argmax(axis=1), y, 70)
    assert np.array_equal(full["confusion"].reshape(-1), ref[:4900]) and full["skipped"] == 0 and full["confusion"].dtype == np.int64
    for got in (small, mid, full):
        assert np.array_equal(got["pairs"], pairs_ref(ref, 70, 20)) and got["counts"].dtype == np.int64
        C = ref[:4900].reshape(70, 70)
        assert np.array_equal(got["counts"], np.concatenate([C.sum(axis=1), C.sum(axis=0), np.diag(C), [0]]))


def test_bad_arguments_return_codes_and_messages():
    from slnlp import _lib, ops
    lib = _lib.load()
    z, y = _device(*make_logp(5, 3, 2.0, 0.6, 1))
    state = ops.temperature_state(0.5, "cuda")
    idx, prob = ops.topk_buffers(5, 2, "cuda")
    p, st = _lib.ptr, _lib.stream_ptr()

    def table(fn, good, cases):
        for i, value, text in cases:
            args = list(good)
            args[i] = value
            rc, msg = fn(*args, st), lib.slnlp_last_error().decode()
            assert rc == 1 and text in msg, (fn.__name__, i, value, rc, msg)

    big = torch.zeros(64, dtype=torch.float64, device="cuda")
    table(lib.slnlp_topk_rows, (p(z), 3, 5, 3, 2, p(state), p(idx), p(prob)),
          [(0, None, "null pointer"), (6, None, "null pointer"), (7, None, "null pointer"), (2, 0, "N=0"), (2, 2 ** 31, "N=2147483648"),
           (3, 0, "V=0"), (3, 2 ** 31, "V=2147483648"), (4, 0, "k=0 outside 1..3"), (4, 4, "k=4 outside 1..3"), (4, -1, "k=-1"),
           (1, 2, "ld=2 is less than V=3"), (1, 2 ** 62, "is no addressable matrix"), (0, p(z) + 2, "misaligned"),
           (5, p(state) + 4, "misaligned"), (6, p(idx) + 2, "misaligned"), (7, p(prob) + 4, "misaligned"),
           (6, p(prob), "idx and prob overlap"), (7, p(idx), "idx and prob overlap"), (6, p(state), "output idx overlaps input beta"),
           (7, p(state), "output prob overlaps input beta"), (6, p(z), "output idx overlaps input logp"),
           (0, p(prob), "output prob overlaps input logp")])              # (the buffers are reinterpreted, nothing is launched)
    wide = torch.zeros(100, 70, dtype=torch.float32, device="cuda")
    rc = lib.slnlp_topk_rows(p(wide), 70, 100, 70, 65, None, p(big), p(big), st)
    assert rc == 1 and "k=65 outside 1..64" in lib.slnlp_last_error().decode()
    assert lib.slnlp_topk_rows(p(z), 3, 5, 3, 2, None, p(idx), p(prob), st) == 0          # beta may be null: beta = 1

    pred = torch.zeros(5, dtype=torch.int32, device="cuda")
    counts = torch.zeros(10, dtype=torch.int32, device="cuda")
    table(lib.slnlp_confusion_matrix, (p(pred), p(y), 5, 3, p(counts)),
          [(0, None, "null pointer"), (1, None, "null pointer"), (4, None, "null pointer"), (2, 0, "N=0"), (2, 2 ** 31, "N=2147483648"),
           (3, 0, "V=0 outside 1..4096"), (3, 4097, "V=4097 outside 1..4096"), (0, p(pred) + 2, "misaligned"), (1, p(y) + 4, "misaligned"),
           (4, p(counts) + 2, "misaligned"), (4, p(pred), "output counts overlaps input pred"), (4, p(y) + 8, "output counts overlaps input y")])

    pairs = torch.zeros(4, 3, dtype=torch.int32, device="cuda")
    work = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert lib.slnlp_confusion_pairs_workspace_bytes(3, 4) == 32
    table(lib.slnlp_confusion_pairs, (p(counts), 3, 4, p(pairs), p(work), 64),
          [(0, None, "null pointer"), (3, None, "null pointer"), (4, None, "null pointer"), (1, 0, "V=0 outside 1..4096"),
           (1, 4097, "V=4097"), (2, 0, "M=0 outside 1..64"), (2, 65, "M=65"), (5, 31, "work_bytes=31 is too small"),
           (0, p(counts) + 2, "misaligned"), (3, p(pairs) + 2, "misaligned"), (4, p(work) + 4, "misaligned"),
           (3, p(counts), "output pairs overlaps input counts"), (4, p(counts), "output work overlaps input counts"),
           (4, p(pairs) + 8, "pairs and work overlap")])
    torch.cuda.synchronize()                                                    # no sticky error: nothing faulted
    assert lib.slnlp_abi_version() == 1
    for k in (0, 4, 2.5, True):
        with pytest.raises(ValueError, match="topk_rows: k="):
            ops.topk_rows(z, k)
    with pytest.raises(ValueError, match="topk_rows"):
        ops.topk_rows(z.double(), 2)
    with pytest.raises(ValueError, match="topk_rows"):
        ops.topk_rows(z, 2, state=state[:8])
    with pytest.raises(ValueError, match="topk_rows"):
        ops.topk_rows(z, 2, out=(idx, prob[:4]))
    with pytest.raises(ValueError, match="confusion_matrix"):
        ops.confusion_matrix(pred.long(), y, 3)
    with pytest.raises(ValueError, match="confusion_matrix"):
        ops.confusion_matrix(pred, y[:4], 3)
    with pytest.raises(ValueError, match="confusion_matrix: V="):
        ops.confusion_matrix(pred, y, 4097)
    with pytest.raises(ValueError, match="confusion_matrix"):
        ops.confusion_matrix(pred, y, 3, out=counts[:9])
    with pytest.raises(ValueError, match="confusion_pairs: M="):
        ops.confusion_pairs(counts, 3, 65)
    with pytest.raises(ValueError, match="confusion_pairs"):
        ops.confusion_pairs(counts[:8], 3, 4)
    with pytest.raises(RuntimeError, match="too small"):
        ops.confusion_pairs(counts, 3, 4, work=work[:16])


# ------------------------------------------------------------------------------------------------------ estimator ----
from test_calibration_gpu import BS, EMA, RNN_CFG, _same, _sd, _strip, make_net, raw_logp  # noqa: E402


@pytest.fixture(scope="module")
def ds():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(120, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


@pytest.fixture(scope="module")
def calibrated(ds):
    return make_net(ds, calibration=TEMPERATURE).partial_fit(ds)


def _check_analysis(net, data, beta, **kw):
    """``net.predict_topk`` and ``net.error_analysis`` against the restatement on the log-probs ``predict_proba`` starts from."""
    from sklearn.metrics import confusion_matrix
    z = raw_logp(net, data)
    V = z.shape[1]
    want_idx, want_prob = topk_ref(z, 3, beta)
    labels, proba = net.predict_topk(data, k=3, **kw)
    assert np.array_equal(labels, net.classes_[want_idx]) and np.abs(proba - want_prob).max() <= BOUND
    assert np.array_equal(labels[:, 0], net.predict(data))
    counts = confusion_ref(z.argmax(axis=1), data.y, V)
    C = counts[:V * V].reshape(V, V)
    got = net.error_analysis(data, pairs=20, top_k=3, **kw)
    assert set(got) == {"classes", "confusion", "report", "macro", "accuracy", "pairs", "topk", "rows"}
    assert got["confusion"].dtype == np.int64 and np.array_equal(got["confusion"], C)
    assert np.array_equal(got["confusion"], confusion_matrix(data.y, net.predict(data), labels=net.classes_))
    report, macro = class_report_ref(C.sum(axis=1), C.sum(axis=0), np.diag(C))
    for k in ("precision", "recall", "f1"):
        assert np.abs(got["report"][k] - report[k]).max() <= 1e-12 and abs(got["macro"][k] - macro[k]) <= 1e-12, k
    assert np.array_equal(got["report"]["support"], report["support"]) and np.array_equal(got["report"]["predicted"], report["predicted"])
    assert got["accuracy"] == float((net.predict(data) == data.y).mean()) and got["rows"] == len(data)
    assert got["pairs"] == [(net.classes_[t], net.classes_[p], int(c)) for t, p, c in pairs_ref(counts, V, 20) if c > 0]
    assert np.array_equal(got["topk"][0], labels) and got["topk"][1].tobytes() == proba.tobytes()
    assert np.array_equal(got["classes"], net.classes_)
    # labels given apart from the dataset's (the model is right nearly everywhere: these fill the cells off the diagonal)
    mixed = np.random.RandomState(0).permutation(np.asarray(data.y))
    counts = confusion_ref(z.argmax(axis=1), mixed, V)
    other = net.error_analysis(data, y=mixed, pairs=64, **kw)
    assert np.array_equal(other["confusion"].reshape(-1), counts[:V * V]) and other["topk"] is None
    assert other["pairs"] == [(net.classes_[t], net.classes_[p], int(c)) for t, p, c in pairs_ref(counts, V, 64) if c > 0]
    assert len(other["pairs"]) > 1 and other["accuracy"] == float((z.argmax(axis=1) == mixed).mean())
    return got


def test_error_analysis_of_a_calibrated_fit(ds, calibrated, monkeypatch):
    net = calibrated
    assert net.temperature_ != 1.0
    before, hist = _sd(net), _strip(net.history)
    pred, proba = net.predict(ds), net.predict_proba(ds)
    on = _check_analysis(net, ds, net.calibration_["beta"])
    off = _check_analysis(net, ds, 1.0, calibrated=False)
    assert np.array_equal(on["confusion"], off["confusion"]) and on["pairs"] == off["pairs"]      # the arg-max never moves
    assert not np.array_equal(on["topk"][1], off["topk"][1])
    # y given apart from the dataset; no top-k; no matrix: then no [V, V] tensor is downloaded, and everything is ONE copy
    V = len(net.classes_)
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(t.numel()) or real(t, *a, **k))
    lean = net.error_analysis(ds, y=ds.y, pairs=7, matrix=False)
    monkeypatch.undo()
    assert copies == [3 * 7 + 3 * V + 1], copies
    assert lean["confusion"] is None and lean["topk"] is None and lean["pairs"] == on["pairs"][:7] and lean["accuracy"] == on["accuracy"]
    assert all(np.array_equal(lean["report"][k], on["report"][k]) for k in on["report"]) and lean["macro"] == on["macro"]
    # neither method leaves a trace
    assert _same(_sd(net), before) and _strip(net.history) == hist
    assert np.array_equal(net.predict(ds), pred) and np.array_equal(net.predict_proba(ds), proba)
    # what is rejected, before anything is launched
    for k in (0, V + 1, 2.5, True, None):
        with pytest.raises(ValueError, match="predict_topk: k="):
            net.predict_topk(ds, k=k)
    for kw in ({"pairs": 0}, {"pairs": 65}, {"top_k": 0}, {"top_k": V + 1}, {"pairs": 1.5}):
        with pytest.raises(ValueError, match="error_analysis: (pairs|top_k)="):
            net.error_analysis(ds, **kw)
    with pytest.raises(ValueError, match="shape"):
        net.error_analysis(ds, y=ds.y[:5])
    wrong = ds.y.copy()
    wrong[3] = V
    with pytest.raises(ValueError, match=f"error_analysis: 1 of 120 labels lie outside the {V} classes of the log-probs"):
        net.error_analysis(ds, y=wrong)


def test_error_analysis_of_a_gru_fit(ds):
    net = make_net(ds, module="model.EncoderDecoderGRUAttn", cfg=RNN_CFG).partial_fit(ds)
    _check_analysis(net, ds, 1.0)


def test_error_analysis_of_a_torch_stepped_fit(ds):
    net = make_net(ds, optimizer="torch.optim.RMSprop", lr=1e-3, calibration=TEMPERATURE)
    assert not net._fused
    net.partial_fit(ds)
    _check_analysis(net, ds, net.calibration_["beta"])


def test_error_analysis_with_ema_weights(ds):
    ema = make_net(ds, weight_averaging=EMA).partial_fit(ds)
    before = _sd(ema)
    live = make_net(ds, seed=3)
    live.module_.load_state_dict(ema.module_.state_dict())
    assert not np.array_equal(raw_logp(ema, ds), raw_logp(live, ds)), "predictions come from the averaged weights"
    _check_analysis(ema, ds, 1.0)
    assert _same(_sd(ema), before), "the live weights came back bit for bit"


# ------------------------------------------------------------------------------------------------------------ CLI ----
def test_cli_writes_the_three_files_only_with_the_key(tmp_path):
    from slnlp import cli
    base = {"seed": 1, "cv": 2, "max_epochs": 2, "batch_size": 16, "test_size": 0.25, "scoring": ["neg_log_loss", "accuracy"],
            "model": "model.Transformer", "model_args": {"embedding_size": 16, "hidden_size": 32, "num_layers": 1, "dropout": 0.1, "num_heads": 2},
            "optimizer_args": {"momentum": 0.9}, "gradient_clipping": {"gradient_clip_value": 0.5}, "grid_args": {"lr": [0.05]},
            "dataset_args": {"synthetic": {"n": 96, "seq_len": 10, "src_vocab": 40, "n_labels": 5, "seed": 4, "min_len": 3}}}
    listing = {}
    for name, extra in (("plain", {}), ("analysed", {"error_analysis": {"pairs": 6, "top_k": 3}})):
        work = tmp_path / name
        gs, _ = cli.run(cli.load_config(None, dict(base, workdir=str(work), **extra)))
        listing[name] = sorted(os.listdir(work))
    new = ["test_class_report.csv", "test_confused_pairs.csv", "test_topk.csv"]
    assert sorted(listing["plain"] + new) == listing["analysed"] and not set(new) & set(listing["plain"])
    assert "test_output.json" in listing["plain"]
    # the contents are the estimator's result on the test split
    est = gs.best_estimator_
    test_data, _ = cli.load_dataset(base).split(0.25, 1)
    want = est.error_analysis(test_data, pairs=6, top_k=3)
    rows = lambda f: list(csv.reader(open(tmp_path / "analysed" / f)))
    rep = rows("test_class_report.csv")
    V = len(est.classes_)
    assert rep[0] == ["class", "name", "precision", "recall", "f1", "support", "predicted"] and len(rep) == V + 2
    for i, r in enumerate(rep[1:-1]):
        assert int(r[0]) == est.classes_[i] and r[1] == test_data.vocab_y.itos[i]
        assert [float(v) for v in r[2:5]] == [want["report"][k][i] for k in ("precision", "recall", "f1")]
        assert [int(v) for v in r[5:]] == [want["report"]["support"][i], want["report"]["predicted"][i]]
    assert rep[-1][0] == "macro" and [float(v) for v in rep[-1][2:5]] == [want["macro"][k] for k in ("precision", "recall", "f1")]
    assert int(rep[-1][5]) == len(test_data) == want["rows"]
    prs = rows("test_confused_pairs.csv")
    assert prs[0] == ["true", "true_name", "predicted", "predicted_name", "count"]
    assert [(int(r[0]), int(r[2]), int(r[4])) for r in prs[1:]] == [(int(t), int(p), c) for t, p, c in want["pairs"]] and len(prs) <= 7
    top = rows("test_topk.csv")
    assert top[0] == ["row", "true", "top1", "top2", "top3", "p1", "p2", "p3"] and len(top) == len(test_data) + 1
    assert np.array_equal(np.array([[int(v) for v in r[2:5]] for r in top[1:]]), want["topk"][0])
    assert np.array_equal(np.array([[float(v) for v in r[5:]] for r in top[1:]]), want["topk"][1])
    assert [int(r[1]) for r in top[1:]] == test_data.y.tolist()
