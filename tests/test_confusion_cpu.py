"""CPU: the host side of the error analysis -- the numpy restatement the GPU tests lean on (tests/confusion_ref.py) against sklearn
and a direct fp64 softmax, the order rules on hand-made rows, ``metrics.class_report``, the options of the estimator and the CLI,
and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

from confusion_ref import class_report_ref, confusion_ref, handmade_rows, pairs_ref, topk_order, topk_ref
from test_calibration_cpu import make_logp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(5, 3, 2.0, 0.6, 1), (257, 70, 8.0, 0.6, 1), (33, 129, 4.0, 0.6, 3), (300, 202, 0.3, 0.2, 7), (2000, 12, 0.3, 0.2, 1),
         (300, 202, 3.0, 0.5, 2)]


def _softmax64(logp, beta=1.0):
    z = beta * logp.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------------------------------------------- restatement ----
@pytest.mark.parametrize("case", CASES)
def test_matrix_and_report_against_sklearn(case):
    from sklearn.metrics import confusion_matrix, precision_recall_fscore_support
    from slnlp import metrics
    logp, y = make_logp(*case)
    V = logp.shape[1]
    pred = logp.argmax(axis=1)
    counts = confusion_ref(pred, y, V)
    C = counts[:V * V].reshape(V, V)
    assert np.array_equal(C, confusion_matrix(y, pred, labels=np.arange(V))) and counts[V * V] == 0
    for report, macro in (class_report_ref(C.sum(axis=1), C.sum(axis=0), np.diag(C)),
                          metrics.class_report(C.sum(axis=1), C.sum(axis=0), np.diag(C).astype(np.int32))):
        p, r, f, s = precision_recall_fscore_support(y, pred, labels=np.arange(V), average=None, zero_division=0)
        assert np.array_equal(report["support"], s) and np.array_equal(report["predicted"], np.bincount(pred, minlength=V))
        assert report["support"].dtype == np.int64 and report["precision"].dtype == np.float64
        for got, want in ((report["precision"], p), (report["recall"], r), (report["f1"], f)):
            assert np.abs(got - want).max() <= 1e-12
        mp, mr, mf, _ = precision_recall_fscore_support(y, pred, labels=np.arange(V), average="macro", zero_division=0)
        assert max(abs(macro["precision"] - mp), abs(macro["recall"] - mr), abs(macro["f1"] - mf)) <= 1e-12


def test_matrix_skips_what_is_no_class():
    logp, y = make_logp(33, 7, 2.0, 0.6, 4)
    pred = logp.argmax(axis=1)
    y[3], y[20], pred[9] = -1, 7, 11
    counts = confusion_ref(pred, y, 7)
    keep = np.ones(33, dtype=bool)
    keep[[3, 9, 20]] = False
    assert counts[49] == 3 and np.array_equal(counts[:49], confusion_ref(pred[keep], y[keep], 7)[:49]) and counts.sum() == 33


@pytest.mark.parametrize("beta", [1.0, 0.16, 6.25])
@pytest.mark.parametrize("case", CASES[:4])
def test_topk_against_a_direct_softmax(case, beta):
    logp, _ = make_logp(*case)
    N, V = logp.shape
    p = _softmax64(logp, beta)
    for k in sorted({k for k in (1, 2, 5, min(V, 64)) if k <= V}):
        idx, prob = topk_ref(logp, k, beta)
        assert idx.shape == prob.shape == (N, k) and idx.dtype == np.int32 and prob.dtype == np.float64
        assert np.array_equal(idx[:, 0], logp.argmax(axis=1))
        assert np.abs(prob - np.take_along_axis(p, idx.astype(np.int64), axis=1)).max() <= 1e-12
        picked = np.take_along_axis(logp, idx.astype(np.int64), axis=1)
        assert (np.diff(picked, axis=1) <= 0).all() and all(len(set(r)) == k for r in idx.tolist())
        ties = np.diff(picked, axis=1) == 0
        assert (np.diff(idx, axis=1)[ties] > 0).all(), "equal values by ascending index"
        # the rest of the row is nowhere larger than the k-th pick
        rest = logp.copy()
        np.put_along_axis(rest, idx.astype(np.int64), -np.inf, axis=1)
        assert (rest.max(axis=1) <= picked[:, -1]).all()


def test_the_tied_case_holds_ties():
    logp, _ = make_logp(300, 202, 0.3, 0.2, 7)
    tied = [i for i, r in enumerate(logp) if len(np.unique(r)) < len(r)]
    assert len(tied) == 3, tied


def test_order_rules_on_a_handmade_row():
    inf = np.inf
    row = np.array([-1.0, np.nan, -0.5, -inf, -0.5, np.nan, -1.0, -0.25, -inf, -0.5], dtype=np.float32)
    assert topk_order(row).tolist() == [1, 5, 7, 2, 4, 9, 0, 6, 3, 8]
    idx, prob = topk_ref(row[None, :], 10)
    assert idx[0].tolist() == [1, 5, 7, 2, 4, 9, 0, 6, 3, 8] and np.isnan(prob).all()
    clean = np.where(np.isnan(row), np.float32(-3.0), row)
    idx, prob = topk_ref(clean[None, :], 10, beta=2.0)
    assert idx[0].tolist() == [7, 2, 4, 9, 0, 6, 1, 5, 3, 8] and idx[0, 0] == np.argmax(clean)
    assert prob[0, -1] == 0.0 and prob[0, -2] == 0.0 and abs(prob.sum() - 1.0) <= 1e-14 and prob[0, 1] == prob[0, 2] == prob[0, 3]
    assert np.isnan(topk_ref(np.array([[0.0, np.inf]], dtype=np.float32), 2)[1]).all()       # a maximum that is not finite
    rows = handmade_rows()
    nan_logp = rows["two_nans_in_a_row"][0]
    idx, prob = topk_ref(nan_logp, 3)
    assert idx[5, :2].tolist() == [1, 4] and np.isnan(prob[5]).all() and not np.isnan(np.delete(prob, 5, axis=0)).any()
    hole, y = rows["one_minus_inf_column"]
    idx, prob = topk_ref(hole, 7)
    assert idx[7, -1] == (y[7] + 1) % 7 and prob[7, -1] == 0.0 and np.isfinite(prob).all()
    five = rows["V70_five_values"][0]
    idx, prob = topk_ref(five, 64)
    assert len(np.unique(five)) == 5 and len(np.unique(prob[0, :14])) == 1 and (np.diff(idx[0, :14]) > 0).all()
    assert prob[0, 13] > prob[0, 14] and abs(prob.sum() + 6 * prob[0, -1] - 1.0) <= 1e-5


@pytest.mark.parametrize("case,cells,cut", [((2000, 12, 0.3, 0.2, 1), 132, (11, 15)), ((300, 202, 3.0, 0.5, 2), 155, (1, 155)),
                                            ((5, 3, 2.0, 0.6, 1), 4, None)])
def test_pairs_against_a_python_sort(case, cells, cut):
    logp, y = make_logp(*case)
    V = logp.shape[1]
    counts = confusion_ref(logp.argmax(axis=1), y, V)
    C = counts[:V * V].reshape(V, V)
    listed = sorted(((int(C[t, p]), t, p) for t in range(V) for p in range(V) if t != p and C[t, p] > 0), key=lambda c: (-c[0], c[1], c[2]))
    assert len(listed) == cells
    for M in (1, 20, 64):
        got = pairs_ref(counts, V, M)
        want = [[t, p, c] for c, t, p in listed[:M]] + [[-1, -1, 0]] * max(0, M - len(listed))
        assert got.dtype == np.int32 and got.tolist() == want
    if cut is not None:                                     # the 64th-largest count and how many cells share it: the tie order cuts
        assert listed[63][0] == cut[0] and sum(c[0] == cut[0] for c in listed) == cut[1]


# -------------------------------------------------------------------------------------------------------- options ----
def test_class_report_arguments():
    from slnlp import metrics
    report, macro = metrics.class_report([3, 0, 2], [2, 1, 2], [2, 0, 1])
    assert report["precision"].tolist() == [1.0, 0.0, 0.5] and report["recall"].tolist() == [2 / 3, 0.0, 0.5]
    assert report["f1"].tolist() == [0.8, 0.0, 0.5] and set(macro) == {"precision", "recall", "f1"}
    assert max(abs(macro["precision"] - 0.5), abs(macro["recall"] - (2 / 3 + 0.5) / 3), abs(macro["f1"] - 1.3 / 3)) <= 1e-15
    assert set(report) == {"precision", "recall", "f1", "support", "predicted"}
    for bad in (([1, 2], [1], [1, 2]), ([1.0], [1.0], [1.0]), ([], [], []), ([[1]], [[1]], [[1]])):
        with pytest.raises(ValueError, match="class_report"):
            metrics.class_report(*bad)


def test_estimator_surface_without_a_gpu():
    from slnlp.net import NeuralNetClassifier
    net = NeuralNetClassifier(module="model.Transformer")
    assert callable(net.predict_topk) and callable(net.error_analysis)
    for call in (net.predict_topk, net.error_analysis):
        with pytest.raises(RuntimeError, match="not initialized"):
            call(None)
    # the options are looked at before anything runs: a fitted estimator's surface, without a module
    net.initialized_, net.classes_ = True, np.arange(6)
    for k in (0, 7, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="predict_topk: k="):
            net.predict_topk(None, k=k)
    for pairs in (0, 65, 1.5, True, None):
        with pytest.raises(ValueError, match="error_analysis: pairs="):
            net.error_analysis(None, pairs=pairs)
    for top_k in (0, 7, 1.5, False):
        with pytest.raises(ValueError, match="error_analysis: top_k="):
            net.error_analysis(None, top_k=top_k)
    net.classes_ = np.arange(100)
    with pytest.raises(ValueError, match="predict_topk: k=65, expected an integer in 1..64"):
        net.predict_topk(None, k=65)


def test_cli_key():
    from slnlp import cli
    assert "error_analysis" in cli.DICT_ARGS
    assert cli.error_analysis_options(None) is None
    assert cli.error_analysis_options({}) == {"pairs": 20, "top_k": 5} == cli.ERROR_ANALYSIS_DEFAULTS
    assert cli.error_analysis_options({"top_k": 3}) == {"pairs": 20, "top_k": 3}
    from slnlp import _lib
    assert cli.ERROR_ANALYSIS_MAX == {"pairs": _lib.PAIRS_MAX, "top_k": _lib.TOPK_MAX}
    for bad in ("yes", 5, ["pairs"], {"pair": 3}, {"pairs": 0}, {"pairs": 65}, {"top_k": 65}, {"top_k": 2.5}, {"pairs": True}):
        with pytest.raises(ValueError, match="error_analysis"):
            cli.error_analysis_options(bad)

    class _Vocab:
        stoi = {"<pad>": 1}

    class _Data:
        vocab_X = vocab_y = _Vocab()
    args = {"model": "model.Transformer", "error_analysis": {"pairs": 3}}
    assert "error_analysis" not in cli.build_net_params(args, _Data(), "cuda")       # the estimator's options are what they were
    import glob
    for f in glob.glob(os.path.join(ROOT, "tests", "golden", "reference_configs", "config-*.yaml")):
        assert cli.load_config(f).get("error_analysis") is None, f


def test_buffers_are_slices_of_one_allocation():
    import __graft_entry__ as ge
    ge.build()
    import torch
    from slnlp import ops
    for N, V, k, M in ((5, 3, 3, 1), (7, 5, 1, 64), (300, 202, 5, 20), (9, 4, None, 2)):
        buf = ops.error_analysis_buffers(N, V, k, M, "cpu")
        flat, at = buf["flat"], buf["at"]
        assert flat.dtype == torch.int32 and flat.dim() == 1
        names = ["confusion", "pairs", "counts", "topk_idx", "topk_prob", "pred", "picked", "rank", "work"]
        assert at["confusion"] == (0, V * V + 1) and at["pairs"] == (V * V + 1, 3 * M) and at["counts"][1] == 3 * V + 1
        end = 0
        for name in names:
            begin, n = at[name]
            assert end <= begin <= end + 1                  # at most one pad entry between neighbours
            end = begin + n
        assert flat.numel() == end and at["topk_prob"][0] % 2 == 0 and at["work"][0] % 2 == 0
        assert buf["work"].numel() == ops.load().slnlp_confusion_pairs_workspace_bytes(V, M) and buf["work"].dtype == torch.uint8
        assert buf["pairs"].shape == (M, 3) and buf["picked"].dtype == torch.float32 and len(buf["score"]) == 4
        if k:
            assert buf["topk_idx"].shape == buf["topk_prob"].shape == (N, k) and buf["topk_prob"].dtype == torch.float64
            assert buf["topk_prob"].data_ptr() % 8 == 0
        else:
            assert buf["topk"] is None and buf["topk_idx"] is None
        assert all(t.data_ptr() >= flat.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= flat.data_ptr() + 4 * flat.numel()
                   for t in (buf["confusion"], buf["pairs"], buf["counts"], buf["pred"], buf["picked"], buf["rank"], buf["work"]))
    for bad in ((0, 3, 1, 1), (5, 4097, 1, 1), (5, 3, 4, 1), (5, 3, 1, 65), (5, 3, 1, 0)):
        with pytest.raises(ValueError, match="error_analysis_buffers"):
            ops.error_analysis_buffers(*bad, "cpu")


# ----------------------------------------------------------------------------------------------------------- C ABI ----
def test_the_entry_points_are_declared_and_bound():
    from slnlp import _lib, ops
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    assert "sklearn" in src[src.index("slnlp_topk_rows:"):src.index("slnlp_confusion_matrix:")], "the header says whose tie order this is not"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                  # the way tests/test_abi.py reads the header
    declared = set(re.findall(r"\b(slnlp_[a-z0-9_]+)\s*\(", src))
    for name, n_args in (("slnlp_topk_rows", 9), ("slnlp_confusion_matrix", 6), ("slnlp_confusion_pairs", 7),
                         ("slnlp_confusion_pairs_workspace_bytes", 2)):
        assert name in declared and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    for macro, value, mirror in (("SLNLP_TOPK_MAX", 64, _lib.TOPK_MAX), ("SLNLP_CONFUSION_MAX_V", 4096, _lib.CONFUSION_MAX_V),
                                 ("SLNLP_PAIRS_MAX", 64, _lib.PAIRS_MAX)):
        (found,), = [re.findall(rf"#define {macro} (\d+)", src)]
        assert int(found) == value == mirror, macro
    assert re.search(r"slnlp_abi_version", src)
    for fn in ("topk_rows", "confusion_matrix", "confusion_pairs", "error_analysis_buffers"):
        assert callable(getattr(ops, fn)), fn
    hip = re.sub(r"//.*", "", open(os.path.join(ROOT, "sign-language-nlp_amd", "csrc", "confusion.hip")).read())
    assert "SLNLP_ZKERNEL" in hip and "zlaunch" in hip and "hipMalloc" not in hip, "argument-pack kernels; the library allocates nothing"
    assert not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", hip) and "atomicAdd(&counts[" in hip, "integer atomics only"
    assert "csrc/confusion.hip" in open(os.path.join(ROOT, "sign-language-nlp_amd", "Makefile")).read()


def test_workspace_bytes_and_its_range():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    lib = _lib.load()
    assert lib.slnlp_abi_version() == 1
    assert lib.slnlp_confusion_pairs_workspace_bytes(12, 64) == 64 * 8                   # one slice
    assert lib.slnlp_confusion_pairs_workspace_bytes(202, 20) == 10 * 20 * 8             # ceil(40804 / 4096) slices
    assert lib.slnlp_confusion_pairs_workspace_bytes(4096, 64) == 1024 * 64 * 8
    for V, M, text in ((0, 1, "V=0"), (4097, 1, "V=4097"), (12, 0, "M=0"), (12, 65, "M=65")):
        assert lib.slnlp_confusion_pairs_workspace_bytes(V, M) == -1 and text in lib.slnlp_last_error().decode()
