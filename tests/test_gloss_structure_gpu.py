"""GPU: gloss structure on the device -- ``slnlp_gloss_structure_begin`` / ``_rows`` / ``_finish`` through ``slnlp.ops`` and
``slnlp.gloss_structure`` against the numpy restatement (tests/gloss_structure_ref.py).  Every integer output EQUALS the
restatement's: no tolerance.  The fp64 outputs are a handful of correctly rounded operations on those integers, on both sides:
they agree to 16 * 2^-53 absolute."""
import functools

import numpy as np
import pytest
import torch

import dup_groups_ref
import gloss_structure_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 63, 64, 65, 257]                              # the wave edge, the block edge, odd N: unaligned rows
CLASSES = [1, 2, 3, 64, 65, 202]                             # the lane-stride edges of the class loop
INTS = ("head", "own", "other", "other_class", "count", "medoid", "class_sum")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dataset(X, L, y):
    from slnlp.data import TokenDataset
    return TokenDataset(X, L, y)


@functools.lru_cache(maxsize=None)
def random_case():
    """The 257 random rows and their unit-cost distances by the restatement, formed once and shared (nobody writes to them)"""
    X, L = dup_groups_ref.random_rows()
    dist, none = ref.distances(X, L)
    return X, L, dist, none


def random_labels(n, C):
    """``arange % C`` with one class index left empty (where there are three or more) and some rows left out"""
    label = (np.arange(n) % C).astype(np.int64)
    if C >= 3:
        label[label == 1] = 0
    label[2::11] = -1
    if n >= 2:
        label[:2] = 0                                        # a class of two rows at least
    return label


@functools.lru_cache(maxsize=None)
def random_want(n, C):
    X, L, dist, none = random_case()
    return ref.integers(dist[:n, :n], none, random_labels(n, C), C)


def _same(got, want, what=""):
    assert got["own"].dtype == np.uint32 and got["other_class"].dtype == np.int32 and got["class_sum"].dtype == np.int64
    for k in INTS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def _run(dist, label, C, max_distance=64, chunks=None):
    """buffers (begin), rows (the matrix uploaded, in ``chunks`` of query rows: default one), finish, download -- on the current stream"""
    from slnlp import ops
    N = dist.shape[0]
    buf = ops.gloss_structure_buffers(N, C, label, max_distance, "cuda")
    for a, b in chunks or [(0, N)]:
        ops.gloss_structure_rows(_dev(dist[a:b]), a, buf)
    ops.gloss_structure_finish(buf)
    return {k: v.copy() for k, v in ops.gloss_structure_download(buf).items()}


@pytest.mark.parametrize("n", SIZES)
def test_ops_equal_the_restatement_on_random_rows(n):
    X, L, dist, none = random_case()
    for C in CLASSES:
        _same(_run(dist[:n, :n], random_labels(n, C), C), random_want(n, C), f"N={n} C={C}")
    if n == 257:                                             # the chunks in any order, a one-row chunk among them; an odd start: unaligned rows
        want, label = random_want(n, 202), random_labels(n, 202)
        assert want["head"][2] > 0 and want["count"][1] == 0 and want["medoid"][1] == -1 and (want["other_class"] >= 0).sum() > 200
        _same(_run(dist, label, 202, chunks=[(200, 257), (0, 100), (100, 101), (101, 200)]), want, "chunks out of order")
        wide = np.where(dist == none, 65535, dist).astype(np.uint16)
        _same(_run(wide, label, 202, chunks=[(0, 129), (129, 257)]), want, "the same distances as uint16")
        _same(_run(wide, label.astype(np.int32), 202, max_distance=1024), want, "int32 labels, another bound")


def test_one_class_under_full_contention():
    same = np.zeros((300, 300), dtype=np.uint8)                                  # 300 identical rows in ONE class: every LDS add meets one address
    got = _run(same, np.zeros(300, dtype=np.int64), 1)
    _same(got, ref.integers(same, 255, np.zeros(300, dtype=np.int64), 1), "300 identical rows")
    assert not got["own"].any() and not got["class_sum"].any() and got["medoid"].tolist() == [0] and (got["other_class"] == -1).all()
    assert got["head"].tolist() == [300, 1, 0, 0, 0, 0, 0, 0]
    X, L = dup_groups_ref.chain_rows(300)
    steps = np.abs(np.arange(300)[:, None] - np.arange(300)[None, :]).astype(np.uint16)      # d(i, j) = |i - j|, stated outright
    assert np.array_equal(steps[:40, :40], ref.distances(X[:40], L[:40], max_len=320)[0])
    got = _run(steps, np.zeros(300, dtype=np.int64), 1, max_distance=320)
    i = np.arange(300, dtype=np.int64)
    own = i * (i + 1) // 2 + (299 - i) * (300 - i) // 2                          # 1 + .. + i below the row, 1 + .. + (299 - i) above
    assert np.array_equal(got["own"], own) and own[149] == own[150] == own.min() and got["medoid"].tolist() == [149]
    assert got["class_sum"].tolist() == [[int(own.sum())]] and got["head"][4] == own.sum()
    # rows 149 and 150 tie (an even number of rows): the lowest row; with 301 rows the middle row 150 is alone
    steps = np.abs(np.arange(301)[:, None] - np.arange(301)[None, :]).astype(np.uint16)
    got = _run(steps, np.zeros(301, dtype=np.int64), 1, max_distance=320)
    i = np.arange(301, dtype=np.int64)
    assert np.array_equal(got["own"], i * (i + 1) // 2 + (300 - i) * (301 - i) // 2) and got["medoid"].tolist() == [150]


@functools.lru_cache(maxsize=None)
def clustered_case():
    X, L, y = ref.clustered_rows(12, 10, 10, 2, seed=4)
    y = y.copy()
    y[37] = y[80]                                            # row 37 (gloss 3 + 2) moved into gloss 8 + 2: the wrong class
    return X, L, y, ref.gloss_structure(X, L, y)


def _report_equals(got, classes, label, want, bound):
    assert np.array_equal(got["classes"], classes) and np.array_equal(got["counts"], want["count"]) and got["counts"].dtype == np.int64
    assert got["medoids"].dtype == np.int64 and np.array_equal(got["medoids"], want["medoid"])
    for k in ("a", "b", "silhouette", "class_distance", "class_silhouette"):
        assert got[k].dtype == np.float64 and np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        assert np.nanmax(np.abs(got[k] - want[k]), initial=0.0) <= ref.TOL, k
    assert abs(got["mean_silhouette"] - want["mean_silhouette"]) <= ref.TOL
    assert got["nearest_class"] == [classes[c].item() if c >= 0 else None for c in want["other_class"]]
    assert (got["flagged"], got["rows"], got["max_distance"]) == (int((label < 0).sum()), len(label), bound)
    wrong = np.flatnonzero((label >= 0) & (want["b"] < want["a"]))
    assert got["misplaced_share"] == len(wrong) / (label >= 0).sum() and len(got["misplaced"]) == min(len(wrong), 50)
    if len(wrong) <= 50:
        assert sorted(m["row"] for m in got["misplaced"]) == wrong.tolist()


def test_gloss_structure_equals_the_restatement_on_clustered_rows():
    import slnlp
    X, L, y, (classes, label, want) = clustered_case()
    assert want["mean_silhouette"] > 0                       # the restatement says the glosses are clusters
    got = slnlp.gloss_structure(_dataset(X, L, y))
    _report_equals(got, classes, label, want, 64)
    assert got["mean_silhouette"] > 0 and got["flagged"] == 0
    rows = {m["row"]: m for m in got["misplaced"]}
    assert 37 in rows and rows[37]["label"] == y[80] and rows[37]["nearest_class"] == 3 + 2 and rows[37]["b"] < rows[37]["a"]
    s = [m["silhouette"] for m in got["misplaced"]]
    assert s == sorted(s) and got["misplaced_share"] == sum(want["b"] < want["a"]) / 120
    pairs = got["closest_pairs"]
    assert len(pairs) == 50 and all(a < b for a, b, *_ in pairs) and [p[2] for p in pairs] == sorted(p[2] for p in pairs)
    assert len(slnlp.gloss_structure(_dataset(X, L, y), top=3)["closest_pairs"]) == 3


def test_medoids_are_a_nearest_prototype_reference_set():
    import slnlp
    X, L, y, (classes, label, want) = clustered_case()
    ds = _dataset(X, L, y)
    medoids = slnlp.gloss_structure(ds)["medoids"]
    assert np.array_equal(medoids, want["medoid"]) and (medoids >= 0).all()
    protos = ds[medoids[medoids >= 0]]
    knn = slnlp.EditKNN(k=1).fit(protos)
    assert np.array_equal(np.asarray(knn.predict(protos)), classes)             # each medoid's own class, one per class in class order


@pytest.mark.parametrize("metric", ["long", "field", "field_gap", "weighted"])
def test_every_metric_equals_its_own_restatement(metric):
    import slnlp
    rs = np.random.RandomState(11)
    n = 130
    if metric == "long":
        X, L = dup_groups_ref.random_rows(n=n, S=128, tokens=3, seed=5)
        L[:40] = rs.randint(0, 6, size=40)                   # short rows: duplicates; long rows: the multi-word recurrence
        L[40:44] = [128, 127, 65, 64]
        X[41, :127] = X[40, :127]                            # rows 40 and 41 differ by one trailing frame
        kw, bound, limit = dict(max_len=128), 128, 128
    else:
        X, L = dup_groups_ref.random_rows(n=n, S=9, tokens=27, seed=6)
        L[:] = rs.randint(0, 5, size=n)
        codes = np.stack([np.arange(30) // 9, np.arange(30) // 3 % 3, np.arange(30) % 3], axis=1).astype(np.int64)      # F = 3; tokens 2..28
        kw = {"field": dict(field_codes=codes), "field_gap": dict(field_codes=codes, gap=2),
              "weighted": dict(field_codes=codes, field_weights=[2, 0, 1], gap=2)}[metric]
        bound, limit = 64 * 3, 64
    y = (np.arange(n) * 5 % 7 + 10).astype(np.int64)
    classes, label, want = ref.gloss_structure(X, L, y, limit=limit, **kw)
    got = slnlp.gloss_structure(_dataset(X, L, y), cap=2 * 50 * n, **kw)        # three chunks of 50, 50 and 30 rows
    _report_equals(got, classes, label, want, bound)
    print(f"{metric}: mean silhouette {got['mean_silhouette']:.4f}, misplaced share {got['misplaced_share']:.3f}")


def test_rows_the_metric_refuses_are_left_out():
    import slnlp
    rs = np.random.RandomState(2)
    X = rs.randint(2, 5, size=(40, 80)).astype(np.int64)     # stride 80: a row of 65 frames fits its row and is refused all the same
    L = rs.randint(0, 6, size=40).astype(np.int64)
    for i in (0, 7, 8, 39):
        X[i], L[i] = X[0], 65
    y = (np.arange(40) % 4).astype(np.int64)
    classes, label, want = ref.gloss_structure(X, L, y)
    assert (label[[0, 7, 8, 39]] == -1).all() and (label >= 0).sum() == 36 and want["head"][2] == 4
    got = slnlp.gloss_structure(_dataset(X, L, y))           # no code is raised: the sentinels lie at pairs with a row left out
    _report_equals(got, classes, label, want, 64)
    assert got["flagged"] == 4 and np.isnan(got["silhouette"][[0, 7, 8, 39]]).all() and got["nearest_class"][7] is None
    keep = np.flatnonzero(label >= 0)                        # they contribute to nobody's sums: the 36 other rows alone give the same
    alone = slnlp.gloss_structure(_dataset(X[keep], L[keep], y[keep]))
    for k in ("a", "b", "silhouette"):
        assert alone[k].tobytes() == got[k][keep].tobytes(), k
    assert alone["class_distance"].tobytes() == got["class_distance"].tobytes()


def test_a_sentinel_at_a_labelled_pair_raises():
    from slnlp import ops
    X, L, dist, none = random_case()
    bad = dist[:65, :65].copy()
    bad[3, 40] = none
    label = random_labels(65, 3)
    assert label[3] >= 0 and label[40] >= 0
    buf = ops.gloss_structure_buffers(65, 3, label, 64, "cuda")
    ops.gloss_structure_finish(ops.gloss_structure_rows(_dev(bad), 0, buf))
    with pytest.raises(RuntimeError, match="code 1: a distance sentinel at a pair of labelled rows"):
        ops.gloss_structure_download(buf)
    label[40] = -1                                           # the same matrix with row 40 left out: fine
    _same(_run(bad, label, 3), ref.integers(bad, none, label, 3), "a sentinel in a column that is left out")
    label[40] = 3                                            # a label outside -1..C-1: found on the device, no index formed from it
    buf = ops.gloss_structure_buffers(65, 3, label, 64, "cuda")
    ops.gloss_structure_finish(ops.gloss_structure_rows(_dev(dist[:65, :65]), 0, buf))
    with pytest.raises(RuntimeError, match="code 2: a label outside -1..2"):
        ops.gloss_structure_download(buf)


def test_the_same_bytes_for_any_chunking_run_and_stream():
    import slnlp
    from slnlp.edit_knn import query_chunks
    X, L, dist, none = random_case()
    y = (np.arange(257) % 7).astype(np.int64)
    ds = _dataset(X, L, y)
    whole = slnlp.gloss_structure(ds)
    chunks = query_chunks(257, 257, 60 * 257)
    assert len(chunks) == 5 and chunks[-1] == (240, 257)     # several chunks, a short last one
    for other in (slnlp.gloss_structure(ds, cap=60 * 257), slnlp.gloss_structure(ds, cap=1), slnlp.gloss_structure(ds, max_len=65, cap=2 * 60 * 257)):
        for k in ("silhouette", "a", "b", "medoids", "class_distance", "class_silhouette", "counts"):
            assert other[k].tobytes() == whole[k].tobytes(), k
        assert other["nearest_class"] == whole["nearest_class"] and other["mean_silhouette"] == whole["mean_silhouette"]
    label = random_labels(257, 7)
    first = _run(dist, label, 7)
    again = _run(dist, label, 7)
    others = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            others.append(_run(dist, label, 7, chunks=[(0, 100), (100, 257)]))
        stream.synchronize()
    for other in (again, *others):
        for k in INTS:
            assert other[k].tobytes() == first[k].tobytes(), k
    _same(first, ref.integers(dist, none, label, 7))


def test_cli_writer_records_unit_and_fitted_weights_side_by_side(tmp_path):
    import csv
    import json
    from slnlp import cli
    X, L, y, (classes, label, want) = clustered_case()
    ds = _dataset(X, L, y)
    cli.save_gloss_structure(ds, cli.gloss_structure_options({"top": 5}), {}, "cuda:0", str(tmp_path))
    out = json.loads((tmp_path / "train_gloss_structure.json").read_text())
    assert out["options"] == {"metric": "unit", "max_len": None, "top": 5} and (out["rows"], out["flagged"], out["max_distance"]) == (120, 0, 64)
    assert abs(out["mean_silhouette"] - want["mean_silhouette"]) <= ref.TOL and len(out["closest_pairs"]) == 5
    assert [c["medoid"] for c in out["per_class"]] == want["medoid"].tolist() and 37 in [m["row"] for m in out["misplaced"]]
    rows = list(csv.reader((tmp_path / "train_gloss_structure_rows.csv").open()))
    assert rows[0][:3] == ["row", "label", "name"] and len(rows) == 121 and sum(int(r[-1]) for r in rows[1:]) == 12
    table = list(csv.reader((tmp_path / "train_gloss_distance.csv").open()))
    assert len(table) == 13 and len(table[1]) == 13 and abs(float(table[1][2]) - want["class_distance"][0, 1]) <= 1e-12
    codes = np.stack([np.arange(32) // 8, np.arange(32) // 2 % 4, np.arange(32) % 2], axis=1).astype(np.int64)      # F = 3 over tokens 0..31
    opts = cli.gloss_structure_options({"metric": "phono"})
    cli.save_gloss_structure(ds, opts, {}, "cuda:0", str(tmp_path), field_codes=codes, field_weights=[2, 0, 1])
    out = json.loads((tmp_path / "train_gloss_structure.json").read_text())
    unit = ref.gloss_structure(X, L, y, field_codes=codes)[2]["mean_silhouette"]
    weighted = ref.gloss_structure(X, L, y, field_codes=codes, field_weights=[2, 0, 1])[2]["mean_silhouette"]
    assert abs(out["mean_silhouette_unit"] - unit) <= ref.TOL and abs(out["mean_silhouette_weighted"] - weighted) <= ref.TOL
    assert out["mean_silhouette"] == out["mean_silhouette_weighted"] and out["field_weights"] == [2, 0, 1] and out["max_distance"] == 192


def test_ops_refuse_what_the_library_would():
    from slnlp import ops
    label = np.array([0, 0, 1, 1, 2, 2, -1, 0])
    buf = ops.gloss_structure_buffers(8, 3, label, 64, "cuda")
    assert buf["shape"] == (8, 3) and buf["label"].dtype == torch.int32 and buf["head"].dtype == torch.int64 and buf["class_sum"].shape == (3, 3)
    torch.cuda.synchronize()
    assert buf["count"].cpu().tolist() == [3, 2, 2] and buf["head"].cpu().tolist() == [7, 0, 1, 0, 0, 0, 0, 0] and not buf["class_sum"].cpu().any()
    good = torch.zeros(2, 8, dtype=torch.uint8, device="cuda")
    for bad in (good[:, :7], good.int(), good.t()[:8, :2], good.cpu(), good[0]):
        with pytest.raises(ValueError, match="dist must be"):
            ops.gloss_structure_rows(bad, 0, buf)
    with pytest.raises(ValueError, match="q0=8"):
        ops.gloss_structure_rows(good, 8, buf)
    with pytest.raises(RuntimeError, match="q0=7"):                              # the library's own check: q0 + nq > N
        ops.gloss_structure_rows(good, 7, buf)
    for foreign in ({"shape": (8, 3, 1)}, ops.dup_groups_buffers(8, "cuda"), None):
        with pytest.raises(ValueError, match="buf must be"):
            ops.gloss_structure_rows(good, 0, foreign)
        with pytest.raises(ValueError, match="buf must be"):
            ops.gloss_structure_finish(foreign)
        with pytest.raises(ValueError, match="buf must be"):
            ops.gloss_structure_download(foreign)
    for kw, says in ((dict(N=0), "N=0"), (dict(C=0), "C=0"), (dict(C=1025), "C=1025"), (dict(max_distance=0), "max_distance=0"),
                     (dict(labels=label[:7]), "labels must be"), (dict(labels=label.astype(np.float32)), "labels must be")):
        with pytest.raises(ValueError, match=says):
            ops.gloss_structure_buffers(**{**dict(N=8, C=3, labels=label, max_distance=64, device="cuda"), **kw})
    with pytest.raises(ValueError, match="reaches 2\\^32"):
        ops.gloss_structure_buffers(2 ** 22, 3, np.zeros(2 ** 22, dtype=np.int32), 1024, "cuda")
