"""CPU: the restatement of the edit-distance neighbour search (tests/edit_knn_ref.py) against hand-checked pairs, the host report
functions on hand-made tables, and every option / argument check of ``EditKNN``, ``split_audit``, ``ops.edit_knn_*`` and the CLI key
that raises before a GPU is needed."""
import numpy as np
import pytest

import edit_knn_ref as ref


# ---------------------------------------------------------------------------------------------------- the restatement ----
def test_hand_checked_pairs():
    assert ref.levenshtein("kitten", "sitting") == 3
    assert ref.levenshtein("flaw", "lawn") == 2
    assert ref.levenshtein("intention", "execution") == 5
    assert ref.levenshtein("", "") == 0
    for L in (1, 5, 64):
        assert ref.levenshtein([], list(range(L))) == L and ref.levenshtein(list(range(L)), []) == L
    assert ref.levenshtein([2 ** 33 + 1, 2 ** 33 + 2], [2 ** 34 + 1, 2 ** 33 + 2]) == 1       # tokens compare as whole int64 values


def test_metric_properties_on_random_rows():
    rs = np.random.RandomState(0)
    rows = [rs.randint(0, 4, size=rs.randint(0, 12)).tolist() for _ in range(40)]
    for a in rows[:10]:
        assert ref.levenshtein(a, a) == 0
    for _ in range(200):
        a, b, c = (rows[i] for i in rs.randint(0, len(rows), size=3))
        ab, bc, ac = ref.levenshtein(a, b), ref.levenshtein(b, c), ref.levenshtein(a, c)
        assert ab == ref.levenshtein(b, a)
        assert ac <= ab + bc
        assert abs(len(a) - len(b)) <= ab <= max(len(a), len(b))


def test_all_pairs_form_equals_the_plain_program():
    """``distances`` forms each row of the two-row program for all references at once: the same integers, 255 for unusable rows,
    and nothing past a row's length matters"""
    rs = np.random.RandomState(1)
    Xq, Xr = rs.randint(0, 3, size=(7, 10)), rs.randint(0, 3, size=(9, 12))
    Lq, Lr = np.array([0, 1, 7, 10, 11, -1, 4]), np.array([12, 0, 5, 65, 3, 9, -1, 1, 12])
    D = ref.distances(Xq, Lq, Xr, Lr)
    assert D.dtype == np.uint8 and D.shape == (7, 9)
    for i in range(7):
        for j in range(9):
            ok = 0 <= Lq[i] <= 10 and 0 <= Lr[j] <= 12
            assert D[i, j] == (ref.levenshtein(Xq[i, :Lq[i]], Xr[j, :Lr[j]]) if ok else 255)
    Xq2, Xr2 = Xq.copy(), Xr.copy()
    for i in range(7):
        Xq2[i, max(Lq[i], 0):] = 99
    for j in range(9):
        Xr2[j, max(Lr[j], 0):] = 98
    assert np.array_equal(D, ref.distances(Xq2, Lq, Xr2, Lr))


def test_the_bit_vector_recurrence_equals_the_plain_program(tmp_path):
    """csrc/edit_myers.hpp -- the recurrence the kernel runs per reference token -- compiled for the host and held to the two-row
    program on 20000 random pairs, a quarter of the lengths at 63 or 64 (tests/edit_myers_check.cpp)"""
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "edit_myers_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-o", exe, os.path.join(here, "edit_myers_check.cpp")], check=True)
    done = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert done.returncode == 0 and done.stdout.strip().endswith("20000 pairs, 0 bad"), done.stdout


def test_selection_order_exclusion_and_eligibility():
    dist = np.array([[3, 1, 1, 255, 1, 0], [255] * 6, [2, 2, 2, 255, 2, 2]], dtype=np.uint8)
    Lq, Lr = np.array([4, 70, 4]), np.array([4, 4, 4, -1, 4, 4])
    res = ref.knn_rows(dist, Lq, Lr, 8, 8, 3, radius=1, exclude=np.array([5, -1, 7]))
    assert res["nbr"][0].tolist() == [[1, 1], [1, 2], [1, 4]]            # the twin 5 is skipped; ties at distance 1 by index
    assert res["rows"][0].tolist() == [3, 3, 1, 0]
    assert res["nbr"][1].tolist() == [[-1, -1]] * 3 and res["rows"][1].tolist() == [0, 0, -1, 1]
    assert res["nbr"][2].tolist() == [[2, 0], [2, 1], [2, 2]] and res["rows"][2].tolist() == [3, 0, 2, 2]     # exclude 7 names nothing
    assert res["head"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    few = ref.knn_rows(dist[:1, :2], Lq[:1], Lr[:2], 8, 8, 4)
    assert few["nbr"][0].tolist() == [[1, 1], [3, 0], [-1, -1], [-1, -1]] and few["rows"][0, 0] == 2


def test_vote_by_hand():
    res = {"rows": np.array([[2, 0, 0, 0], [0, 0, -1, 0], [0, 0, -1, 1]], dtype=np.int32),
           "nbr": np.array([[[0, 1], [2, 0]], [[-1, -1]] * 2, [[-1, -1]] * 2], dtype=np.int32)}
    prior = np.array([0.5, 0.25, 0.25])
    z, bad = ref.knn_logp(res, [4, 4, 4], [4, 2], [2, 0], prior, weights="distance", tau=1.0, normalize=True, lam=1.0)
    w = np.exp(-2.0 / 4.0)
    assert np.allclose(np.exp(z[0].astype(np.float64)), np.array([1.0 + 0.5, 0.25, w + 0.25]) / (1.0 + w + 1.0), rtol=1e-6) and bad == 0
    assert np.allclose(np.exp(z[1].astype(np.float64)), prior, rtol=1e-6) and np.isnan(z[2]).all()
    z, bad = ref.knn_logp(res, [4, 4, 4], [4, 2], [2, 9], prior, weights="uniform", lam=1.0)
    assert bad == 1 and np.allclose(np.exp(z[0].astype(np.float64)), np.array([0.5, 0.25, 1.25]) / 2.0, rtol=1e-6)
    assert np.allclose(ref.prior_of([0, 0, 2], 3), [3 / 6, 1 / 6, 2 / 6])


# --------------------------------------------------------------------------------------------------------- the reports ----
def _tables():
    """Five held-out rows against train rows labelled a b a c: an exact twin with another label, an exact twin, a near one with
    another label, a far one, and a query with no eligible reference"""
    rows = np.array([[2, 1, 0, 0], [2, 2, 0, 0], [2, 1, 2, 0], [2, 0, 9, 0], [0, 0, -1, 1]], dtype=np.int32)
    nbr = np.array([[[0, 1], [3, 0]], [[0, 2], [1, 0]], [[2, 3], [5, 1]], [[9, 0], [9, 1]], [[-1, -1], [-1, -1]]], dtype=np.int32)
    return rows, nbr, np.array(["a", "a", "a", "b", "c"], dtype=object), np.array(["a", "b", "a", "c"], dtype=object)


def test_split_audit_report_by_hand():
    from slnlp import metrics
    rows, nbr, yq, yr = _tables()
    res = metrics.split_audit_report(rows, nbr, yq, yr, 2, 10, head=np.array([1, 3, 0, 0, 0, 0, 0, 0]))
    assert (res["rows"], res["exact_duplicates"], res["near_duplicates"], res["conflicting"], res["conflicting_exact"]) == (5, 2, 3, 2, 1)
    assert res["nearest_hist"].shape == (66,) and res["nearest_hist"].dtype == np.int64
    assert res["nearest_hist"][[0, 2, 9, 65]].tolist() == [2, 1, 1, 1] and res["nearest_hist"].sum() == 5
    assert res["per_class"]["label"].tolist() == ["a", "b", "c"] and res["per_class"]["support"].tolist() == [3, 1, 1]
    assert res["per_class"]["duplicated"].tolist() == [3, 0, 0] and res["per_class"]["conflicting"].tolist() == [2, 0, 0]
    # smallest distance first, ties by query then reference row; only listed neighbours within the radius
    assert res["pairs"] == [(0, 1, 0, "a", "b"), (1, 2, 0, "a", "a"), (1, 0, 1, "a", "a"), (2, 3, 2, "a", "c")]
    assert metrics.split_audit_report(rows, nbr, yq, yr, 2, 2)["pairs"] == res["pairs"][:2]
    assert res["duplicated"].tolist() == [True, True, True, False, False]
    assert (res["flagged_queries"], res["flagged_references"]) == (1, 3)
    assert metrics.split_audit_report(rows, nbr, yq, yr, 0, 10)["near_duplicates"] == 2
    ints = metrics.split_audit_report(rows, nbr, np.array([0, 0, 0, 1, 2]), np.array([0, 1, 0, 2]), 2, 10)
    assert ints["pairs"][0] == (0, 1, 0, 0, 1) and ints["flagged_references"] == 0
    with pytest.raises(ValueError, match="split_audit_report: radius=65"):
        metrics.split_audit_report(rows, nbr, yq, yr, 65, 10)
    with pytest.raises(ValueError, match="split_audit_report: top=-1"):
        metrics.split_audit_report(rows, nbr, yq, yr, 2, -1)
    with pytest.raises(ValueError, match="split_audit_report: rows int32"):
        metrics.split_audit_report(rows[:, :3], nbr, yq, yr, 2, 10)
    with pytest.raises(ValueError, match="y_query has shape"):
        metrics.split_audit_report(rows, nbr, yq[:4], yr, 2, 10)


def test_knn_report_by_hand():
    from slnlp import metrics
    rows, nbr, yq, yr = _tables()
    res = metrics.knn_report(rows, nbr, yq, yr, head=np.array([1, 3, 2, 0, 0, 0, 0, 0]))
    assert (res["rows"], res["k"], res["flagged_queries"], res["no_neighbour"]) == (5, 2, 1, 0)
    assert res["listed"].tolist() == [4, 4] and res["agreement"].tolist() == [0.25, 0.75] and res["accuracy_1nn"] == 0.25
    assert res["mean_nearest"] == pytest.approx(11 / 4) and res["mean_distance"].tolist() == [11 / 4, 18 / 4]
    assert np.array_equal(res["nearest_hist"], metrics.split_audit_report(rows, nbr, yq, yr, 2, 0)["nearest_hist"])
    assert (res["flagged_references"], res["bad_labels"]) == (3, 2)


# ----------------------------------------------------------------------------------- checks that need no GPU ----
def test_exported():
    import slnlp
    from slnlp import edit_knn
    assert slnlp.EditKNN is edit_knn.EditKNN and slnlp.split_audit is edit_knn.split_audit
    assert {"EditKNN", "split_audit"} <= set(slnlp.__all__)


def test_estimator_options():
    import slnlp
    from sklearn.base import clone
    knn = slnlp.EditKNN()
    assert knn.get_params() == dict(k=5, weights="distance", tau=1.0, normalize=True, smoothing=1.0, device=None)
    assert clone(slnlp.EditKNN(k=3, weights="uniform")).get_params()["k"] == 3
    assert knn.calibration_ is None and knn.temperature_ == 1.0 and not knn.initialized_
    for kw, text in ((dict(k=0), "k=0"), (dict(k=65), "k=65"), (dict(k=True), "k=True"), (dict(weights="rank"), "weights='rank'"),
                     (dict(tau=0.0), "tau=0.0"), (dict(tau=float("inf")), "tau=inf"), (dict(normalize=1), "normalize=1"),
                     (dict(smoothing=0), "smoothing=0"), (dict(smoothing=float("nan")), "smoothing=nan")):
        with pytest.raises(ValueError, match=f"EditKNN: {text}"):
            slnlp.EditKNN(**kw)
    with pytest.raises(ValueError, match="expected a cuda device"):
        slnlp.EditKNN(device="cpu")
    with pytest.raises(RuntimeError, match="not initialized"):
        knn.predict_proba(_dataset())
    with pytest.raises(RuntimeError, match="not initialized"):
        knn.leave_one_out()


def _dataset(n=6, S=5, lengths=None, y=None):
    from slnlp.data import TokenDataset
    rs = np.random.RandomState(2)
    return TokenDataset(rs.randint(2, 9, size=(n, S)), rs.randint(1, S + 1, size=n) if lengths is None else lengths,
                        rs.randint(0, 3, size=n) if y is None else y)


def test_fit_refuses_before_the_gpu():
    import slnlp
    with pytest.raises(ValueError, match=r"EditKNN.fit: 2 of 6 rows have a length outside 0..5 \(first: row 1, length 6\).*refused, not truncated"):
        slnlp.EditKNN().fit(_dataset(lengths=[1, 6, 2, -1, 5, 0]))
    from slnlp.data import TokenDataset
    long = TokenDataset(np.zeros((2, 70), dtype=np.int64), [64, 65], [0, 1])
    with pytest.raises(ValueError, match=r"1 of 2 rows have a length outside 0..64 \(first: row 1, length 65\)"):
        slnlp.EditKNN().fit(long)
    with pytest.raises(ValueError, match="EditKNN.fit: 1 of 6 labels lie outside"):
        slnlp.EditKNN().fit(_dataset(y=[0, 1, 2, -1, 0, 1]))
    with pytest.raises(TypeError, match="TokenDataset"):
        slnlp.EditKNN().fit(np.zeros((3, 4)))
    knn = slnlp.EditKNN()
    knn.k = 99                                               # set_params goes past __init__: fit checks again
    with pytest.raises(ValueError, match="EditKNN: k=99"):
        knn.fit(_dataset())


def test_leave_one_out_refuses_other_data():
    """The refusal compares length, labels, lengths and ids, before anything touches the device"""
    import copy
    import slnlp
    own = _dataset()
    knn = slnlp.EditKNN()
    knn.rows_, knn.dataset_, knn.initialized_, knn._loo, knn.classes_ = len(own), own, True, True, np.arange(3)   # a sibling's host state
    same = copy.deepcopy(own)
    knn._refuse_other_data(own)
    knn._refuse_other_data(same)                             # equal contents pass
    other = copy.deepcopy(own)
    other.ids[2, 0] += 1
    with pytest.raises(ValueError, match=r"exist only for the 6 rows that were fitted on, in their order; got a dataset of 6 rows with other contents"):
        knn._forward_logp(other, lambda z, y: z)
    with pytest.raises(ValueError, match=r"got a dataset of 4 rows \(the fitted EditKNN predicts new rows\)"):
        knn.kneighbors(own[np.arange(4)])
    with pytest.raises(NotImplementedError, match="occluded variants"):
        knn.attribute(own)


def test_query_chunks_cover_every_row_once_under_the_cap():
    from slnlp.edit_knn import SCRATCH_PAIRS, query_chunks
    for nq, nr, cap in ((1, 1, 1), (10, 4, 12), (100, 300, 2100), (7, 50, 10), (4000, 4000, SCRATCH_PAIRS), (16384, 4000, 1 << 24),
                        (100000, 30000, SCRATCH_PAIRS)):
        chunks = query_chunks(nq, nr, cap)
        assert chunks[0][0] == 0 and chunks[-1][1] == nq and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        assert all(a < b for a, b in chunks)
        assert all((b - a) * nr <= cap or b - a == 1 for a, b in chunks)
    assert query_chunks(4000, 4000) == [(0, 4000)] and len(query_chunks(10, 4, 12)) == 4
    assert SCRATCH_PAIRS <= 2 ** 31
    with pytest.raises(ValueError, match="query_chunks: nq=0"):
        query_chunks(0, 4)


def test_split_audit_argument_checks():
    import slnlp
    ds = _dataset()
    with pytest.raises(TypeError, match="split_audit: test must be a non-empty"):
        slnlp.split_audit(ds, None)
    with pytest.raises(ValueError, match="split_audit: radius=65"):
        slnlp.split_audit(ds, ds, radius=65)
    with pytest.raises(ValueError, match="split_audit: top=-1"):
        slnlp.split_audit(ds, ds, top=-1)
    with pytest.raises(TypeError, match="split_audit: judge must be a LogProbJudge"):
        slnlp.split_audit(ds, ds, judge=object())
    with pytest.raises(ValueError, match="expected a cuda device"):
        slnlp.split_audit(ds, ds, device="cpu")


def test_ops_argument_checks():
    import torch
    from slnlp import ops
    with pytest.raises(ValueError, match="edit_knn_buffers: nq=0"):
        ops.edit_knn_buffers(0, 5, "cpu")
    with pytest.raises(ValueError, match="edit_knn_buffers: k=65"):
        ops.edit_knn_buffers(4, 65, "cpu")
    buf = ops.edit_knn_buffers(3, 2, "cpu")                  # the layout needs no GPU
    assert buf["shape"] == (3, 2) and buf["head"].shape == (8,) and buf["rows"].shape == (3, 4) and buf["nbr"].shape == (3, 2, 2)
    assert list(buf["packed"].at) == ["head", "rows", "nbr"] and buf["flat"].numel() * 4 == 64 + 48 + 48
    got = ops.edit_knn_download(buf)
    assert list(got) == ["head", "rows", "nbr"] and list(ops.edit_knn_download(buf, neighbours=False)) == ["head", "rows"]
    X, L = torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    for k in (0, 65, 2.0):
        with pytest.raises(ValueError, match="edit_knn_rows: k="):
            ops.edit_knn_rows(X, L, X, L, k)
    with pytest.raises(ValueError, match="edit_knn_rows: radius=-1"):
        ops.edit_knn_rows(X, L, X, L, 2, radius=-1)
    prior = torch.full((3,), 1 / 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="edit_knn_logp: weights='rank'"):
        ops.edit_knn_logp(buf, L, L, L, prior, weights="rank")
    with pytest.raises(ValueError, match="edit_knn_logp: tau=0"):
        ops.edit_knn_logp(buf, L, L, L, prior, tau=0)
    with pytest.raises(ValueError, match="edit_knn_logp: lam=-1"):
        ops.edit_knn_logp(buf, L, L, L, prior, lam=-1)
    with pytest.raises(ValueError, match="edit_knn_logp: buf must be edit_knn_buffers"):
        ops.edit_knn_logp({"shape": (3,)}, L, L, L, prior)
    with pytest.raises(ValueError, match="edit_knn_download: buf must be"):
        ops.edit_knn_download(None)


def test_cli_key():
    from slnlp import cli
    assert cli.baseline_options(None) is None and "baseline" in cli.DICT_ARGS
    assert cli.baseline_options({}) == {"k": 5, "weights": "distance", "tau": 1.0, "normalize": True, "smoothing": 1.0, "radius": 2, "top": 50}
    assert cli.baseline_options({"k": 1, "radius": 0})["k"] == 1
    for bad, text in ((5, "expected a dict"), ({"neighbours": 3}, "unknown keys"), ({"k": 0}, "k=0"), ({"k": True}, "k=True"),
                      ({"weights": "rank"}, "weights='rank'"), ({"tau": 0}, "tau=0"), ({"smoothing": "1"}, "smoothing='1'"),
                      ({"normalize": 1}, "normalize=1"), ({"radius": 65}, "radius=65"), ({"top": -1}, "top=-1")):
        with pytest.raises(ValueError, match=f"baseline.*{text}"):
            cli.baseline_options(bad)
    assert "baseline:" in cli.__doc__ and "test_split_audit.json" in cli.__doc__
