"""CPU: gloss structure -- the numpy restatement (tests/gloss_structure_ref.py) against sklearn's ``silhouette_samples`` and a plain
double loop, its conventions at the edges, the host's report builder on synthetic integers, the argument checks of the three
``slnlp_gloss_structure_*`` entry points (codes and messages, no launch, no GPU) and the CLI key."""
import ctypes as C

import numpy as np
import pytest

import dup_groups_ref
import gloss_structure_ref as ref


def _silhouette_case(which):
    if which == "random":
        X, L = dup_groups_ref.random_rows()
        y = np.arange(len(L)) % 3
    else:
        X, L, y = dup_groups_ref.planted_rows()
    dist, none = ref.distances(X, L)
    classes, label = np.unique(y, return_inverse=True)
    return dist, none, label.reshape(-1), len(classes)


# ------------------------------------------------------------------------------------------- the restatement ----
@pytest.mark.parametrize("which", ["random", "planted"])
def test_restatement_equals_sklearn(which):
    from sklearn.metrics import silhouette_samples
    dist, none, label, Cn = _silhouette_case(which)
    got = ref.structure(dist, none, label, Cn)
    want = silhouette_samples(dist.astype(np.float64), label, metric="precomputed")
    worst = float(np.abs(got["silhouette"] - want).max())
    print(f"{which}: {len(label)} rows, {Cn} classes, max |s - sklearn| = {worst}")
    assert worst <= ref.TOL
    assert abs(got["mean_silhouette"] - want.mean()) <= ref.TOL


def test_medoids_and_class_distances_equal_a_double_loop():
    X, L = dup_groups_ref.random_rows()
    X, L = X[:40], L[:40]
    label = (np.arange(40) * 7 % 5).astype(np.int64)
    label[[3, 17]] = -1
    dist, none = ref.distances(X, L)
    got = ref.structure(dist, none, label, 5)
    sums, own = np.zeros((5, 5), dtype=np.int64), np.zeros(40, dtype=np.int64)
    for i in range(40):
        for j in range(40):
            if i != j and label[i] >= 0 and label[j] >= 0:
                sums[label[i], label[j]] += int(dist[i, j])
                if label[i] == label[j]:
                    own[i] += int(dist[i, j])
    assert np.array_equal(got["class_sum"], sums) and np.array_equal(sums, sums.T) and np.array_equal(got["own"], own)
    n = np.bincount(label[label >= 0], minlength=5)
    for a in range(5):
        rows = [i for i in range(40) if label[i] == a]
        assert got["medoid"][a] == min(rows, key=lambda i: (own[i], i))
        for b in range(5):
            pairs = n[a] * (n[b] - (a == b))
            assert got["class_distance"][a, b] == sums[a, b] / pairs
    assert got["head"].tolist() == [38, 5, 2, 0, int(own.sum()), 0, 0, 0]
    assert np.isnan(got["silhouette"][[3, 17]]).all() and not got["own"][[3, 17]].any() and (got["other_class"][[3, 17]] == -1).all()


def test_conventions_at_the_edges():
    d = np.array([[0, 2, 4, 6], [2, 0, 2, 4], [4, 2, 0, 2], [6, 4, 2, 0]], dtype=np.uint8)
    one = ref.structure(d, 255, np.array([0, 0, 0, 1]), 2)                       # a class of one row: s = 0, its own medoid
    assert one["silhouette"][3] == 0 and one["medoid"].tolist() == [1, 3] and one["own"][3] == 0 and one["a"][3] == 0
    assert one["silhouette"][0] == (6 - 3) / 6 and np.isnan(one["class_distance"][1, 1])
    only = ref.structure(d, 255, np.zeros(4, dtype=np.int64), 1)                 # one class only: no other class, s = 0
    assert (only["other_class"] == -1).all() and not only["other"].any() and not only["silhouette"].any()
    assert only["medoid"].tolist() == [1] and only["class_sum"].tolist() == [[40]]           # rows 1 and 2 tie at 8: the lowest row
    same = ref.structure(np.zeros((6, 6), dtype=np.uint8), 255, np.arange(6) % 2, 2)         # all rows identical: max(a, b) = 0
    assert not same["silhouette"].any() and same["mean_silhouette"] == 0 and same["medoid"].tolist() == [0, 1]
    assert same["other_class"].tolist() == [1, 0, 1, 0, 1, 0]
    gap = ref.structure(d, 255, np.array([0, 0, 2, 2]), 3)                       # an empty class index
    assert gap["medoid"].tolist() == [0, -1, 2] and gap["count"].tolist() == [2, 0, 2] and gap["head"][1] == 2
    assert np.isnan(gap["class_distance"][1]).all() and np.isnan(gap["class_distance"][:, 1]).all() and np.isnan(gap["class_silhouette"][1])
    assert not np.isnan(gap["class_distance"][[0, 0, 2, 2], [0, 2, 0, 2]]).any() and (gap["other_class"] != 1).all()
    # ties on a hand-made matrix: row 0 (class 0) is at mean distance 3 from class 1 (rows 1, 2: 2 + 4) and from class 2 (row 3: 3)
    t = np.array([[0, 2, 4, 3], [2, 0, 9, 9], [4, 9, 0, 9], [3, 9, 9, 0]], dtype=np.uint8)
    tie = ref.structure(t, 255, np.array([0, 1, 1, 2]), 3)
    assert tie["other_class"][0] == 1 and tie["other"][0] == 6                   # 6 / 2 == 3 / 1: the lower class
    flip = ref.structure(t, 255, np.array([0, 2, 2, 1]), 3)                      # the same sums, the classes renamed
    assert flip["other_class"][0] == 1 and flip["other"][0] == 3
    with pytest.raises(AssertionError, match="sentinel"):
        ref.integers(np.array([[0, 255], [255, 0]], dtype=np.uint8), 255, np.array([0, 1]), 2)
    left = ref.integers(np.array([[0, 255], [255, 255]], dtype=np.uint8), 255, np.array([0, -1]), 1)     # a refused row, left out: fine
    assert left["head"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]


def test_clustered_rows_are_clusters():
    X, L, y = ref.clustered_rows(12, 10, 10, 2, seed=4)
    assert X.shape == (120, 12) and L.min() >= 8 and L.max() <= 12 and np.array_equal(np.unique(y), np.arange(12) + 2)
    classes, label, want = ref.gloss_structure(X, L, y)
    assert want["mean_silhouette"] > 0 and (want["class_silhouette"] > 0).all()


# ------------------------------------------------------------------------------------------- the report builder ----
def test_host_values_equal_the_restatement():
    from slnlp import gloss_structure as gs
    dist, none, label, Cn = _silhouette_case("random")
    label = label.copy()
    label[[5, 100]] = -1
    want = ref.structure(dist, none, label, Cn + 1)                             # an empty class index too
    a, b, s, cd = gs.structure_values(label, want["count"], want["own"], want["other"], want["other_class"], want["class_sum"])
    for got, key in ((a, "a"), (b, "b"), (s, "silhouette"), (cd, "class_distance")):
        assert np.array_equal(np.isnan(got), np.isnan(want[key])), key
        assert np.nanmax(np.abs(got - want[key])) <= ref.TOL, key


def test_report_builder_orders_and_caps():
    from slnlp import gloss_structure as gs
    classes = np.array([10, 20, 30, 40])
    label = np.array([0, 0, 0, 1, 1, 1, 2, 2, -1])
    got = {"count": np.array([3, 3, 2, 0]), "medoid": np.array([1, 3, 6, -1]),
           "own": np.array([4, 2, 6, 12, 2, 8, 5, 5, 0], dtype=np.uint32), "other": np.array([9, 3, 2, 3, 9, 6, 30, 3, 0], dtype=np.uint32),
           "other_class": np.array([1, 1, 2, 0, 0, 2, 0, 1, -1]),
           "class_sum": np.array([[12, 27, 6, 0], [27, 22, 12, 0], [6, 12, 10, 0], [0, 0, 0, 0]])}
    rep = gs.structure_report(classes, label, got, 64, top=2)
    assert rep["a"][:3].tolist() == [2.0, 1.0, 3.0] and rep["b"][:3].tolist() == [3.0, 1.0, 1.0] and np.isnan(rep["silhouette"][8])
    assert rep["silhouette"][:3].tolist() == [1 / 3, 0.0, -2 / 3]
    # b < a: rows 2 (s = -2/3), 3 (a 6, b 1: -5/6), 5 (a 4, b 3: -1/4), 7 (a 5, b 1: -4/5); the most negative first, two kept
    assert [m["row"] for m in rep["misplaced"]] == [3, 7] and rep["misplaced_share"] == 4 / 8
    assert rep["misplaced"][0] == {"row": 3, "label": 20, "nearest_class": 10, "a": 6.0, "b": 1.0, "silhouette": -5 / 6}
    assert rep["nearest_class"] == [20, 20, 30, 10, 10, 30, 10, 20, None]
    assert rep["closest_pairs"] == [(10, 30, 1.0, 3, 2), (20, 30, 2.0, 3, 2)]    # (10, 20) is at 3.0; class 40 is empty: in no pair
    assert len(gs.structure_report(classes, label, got, 64, top=50)["closest_pairs"]) == 3
    assert rep["class_distance"][0, 0] == 2.0 and np.isnan(rep["class_distance"][3]).all() and np.isnan(rep["class_silhouette"][3])
    assert rep["medoids"].dtype == np.int64 and rep["medoids"].tolist() == [1, 3, 6, -1] and rep["counts"].tolist() == [3, 3, 2, 0]
    assert (rep["flagged"], rep["rows"], rep["max_distance"]) == (1, 9, 64)
    assert rep["mean_silhouette"] == rep["silhouette"][:8].mean() and rep["class_silhouette"][2] == rep["silhouette"][6:8].mean()
    assert gs.structure_report(classes, label, got, 64, top=0)["misplaced"] == []


def test_public_function_checks_its_arguments_before_the_device():
    import slnlp
    from slnlp import gloss_structure as gs
    from slnlp.data import TokenDataset
    assert "gloss_structure" in slnlp.__all__ and callable(slnlp.gloss_structure) and callable(gs.gloss_structure)
    assert slnlp.gloss_structure is gs                       # the module carries the function's name and calls it
    X, L, y = dup_groups_ref.planted_rows()
    ds = TokenDataset(X, L, y)
    codes = np.arange(50 * 3).reshape(50, 3) % 5
    for kw, says in ((dict(max_len=64), "max_len=64"), (dict(max_len=128, field_codes=codes), "limited to 64 frames"),
                     (dict(gap=1), "without field_codes"), (dict(field_weights=[1, 1, 1]), "without field_codes"),
                     (dict(field_codes=codes, gap=4), "gap=4"), (dict(cap=0), "cap=0"), (dict(top=-1), "top=-1"), (dict(device="cpu"), "cuda device")):
        with pytest.raises(ValueError, match=f"gloss_structure.*{says}|{says}"):
            slnlp.gloss_structure(ds, **kw)
    with pytest.raises(TypeError, match="TokenDataset"):
        slnlp.gloss_structure(np.zeros((3, 3)))
    many = TokenDataset(np.full((1025, 2), 3, dtype=np.int64), np.full(1025, 2, dtype=np.int64), np.arange(1025))
    with pytest.raises(ValueError, match="1025 classes, at most 1024"):
        slnlp.gloss_structure(many)


# ------------------------------------------------------------------------------------------------------------ ABI ----
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    return _lib.load()


def test_entry_points_validate_before_they_touch_a_device(lib):
    """slnlp_gloss_structure_begin / _rows / _finish check pointers, counts, classes, width, the 32-bit bound, alignment and overlaps
    first: codes and messages, no launch, no GPU needed."""
    INVALID = 1                                                                  # SLNLP_ERR_INVALID_ARG
    mem = (C.c_int64 * 8192)()
    base = C.cast(mem, C.c_void_p).value                                         # non-null addresses: nothing below gets as far as reading them
    dist, label, count, medoid, own, other, other_class = (base + k * 1024 for k in range(7))
    head, med_sum, class_sum = base + 8192, base + 9216, base + 16384           # C = 8: class_sum takes 512 bytes
    says = lambda: lib.slnlp_last_error().decode()
    N, Cn = 64, 8

    def begin(label=label, N=N, C=Cn, max_distance=64, count=count, class_sum=class_sum, med_sum=med_sum, medoid=medoid, head=head):
        return lib.slnlp_gloss_structure_begin(label, N, C, max_distance, count, class_sum, med_sum, medoid, head, None)

    def rows(dist=dist, width=1, nq=8, N=N, q0=0, label=label, C=Cn, count=count, own=own, other=other, other_class=other_class,
             class_sum=class_sum, med_sum=med_sum, head=head):
        return lib.slnlp_gloss_structure_rows(dist, width, nq, N, q0, label, C, count, own, other, other_class, class_sum, med_sum, head, None)

    def finish(label=label, own=own, med_sum=med_sum, N=N, C=Cn, medoid=medoid, head=head):
        return lib.slnlp_gloss_structure_finish(label, own, med_sum, N, C, medoid, head, None)

    for call, name in ((begin, "gloss_structure_begin"), (rows, "gloss_structure_rows"), (finish, "gloss_structure_finish")):
        for arg in ("label", "med_sum", "head"):
            assert call(**{arg: None}) == INVALID and f"{name}: null pointer" in says()
        for bad in (0, -1, 2 ** 30 + 1):
            assert call(N=bad) == INVALID and "outside 1..1073741824" in says()
        for bad in (0, 1025, -1):
            assert call(C=bad) == INVALID and f"{name}: C={bad} outside 1..1024" in says()
        assert call(head=head + 4) == INVALID and "misaligned" in says()
        assert call(label=label + 2) == INVALID and "misaligned" in says()
        assert call(med_sum=med_sum + 4) == INVALID and "misaligned" in says()
    assert begin(max_distance=2 ** 26, N=64) == INVALID and "max_distance=67108864" in says()
    assert begin(max_distance=64, N=2 ** 26) == INVALID and "reaches 2^32" in says()            # 64 * 2^26 = 2^32 exactly
    assert begin(max_distance=1024, N=2 ** 22) == INVALID and "reaches 2^32" in says()
    assert begin(max_distance=0) == INVALID and "max_distance=0" in says()
    assert begin(count=None) == INVALID and begin(medoid=None) == INVALID and begin(class_sum=None) == INVALID
    assert begin(count=medoid + 4 * (Cn - 1)) == INVALID and "outputs count and medoid overlap" in says()
    assert begin(class_sum=med_sum - 8) == INVALID and "outputs class_sum and med_sum overlap" in says()
    assert begin(head=label + 8) == INVALID and "output head overlaps input label" in says()
    assert rows(dist=None) == INVALID and "gloss_structure_rows: null pointer" in says()
    for bad in (0, 3, 4, -1):
        assert rows(width=bad) == INVALID and f"width={bad}" in says()
    for bad in (0, -3, 2 ** 30 + 1):
        assert rows(nq=bad) == INVALID and "nq=" in says()
    assert rows(nq=8, q0=57) == INVALID and "q0=57" in says()                    # q0 + nq > N
    assert rows(q0=-1) == INVALID and "q0=-1" in says()
    assert rows(nq=65) == INVALID
    far = {k: base + ((i + 1) << 40) for i, k in enumerate(("label", "own", "other", "other_class"))}
    assert rows(nq=2 ** 16, N=2 ** 16, **far) == INVALID and "pairs" in says()
    assert rows(width=2, dist=dist + 1) == INVALID and "misaligned" in says()
    assert rows(own=own + 1) == INVALID and "misaligned" in says()
    assert rows(other=own + 4 * (N - 1)) == INVALID and "outputs own and other overlap" in says()
    assert rows(other_class=other) == INVALID and "outputs other and other_class overlap" in says()
    assert rows(own=dist + 8 * N - 4) == INVALID and "output own overlaps input dist" in says()
    assert rows(width=2, own=dist + 2 * 8 * N - 4) == INVALID and "output own overlaps input dist" in says()
    assert rows(head=label + 8) == INVALID and "output head overlaps input label" in says()
    assert rows(class_sum=count) == INVALID and "output class_sum overlaps input count" in says()
    assert finish(medoid=None) == INVALID and "gloss_structure_finish: null pointer" in says()
    assert finish(medoid=own + 4) == INVALID and "output medoid overlaps input own" in says()
    assert finish(head=med_sum) == INVALID and "output head overlaps input med_sum" in says()
    assert finish(medoid=medoid + 1) == INVALID and "misaligned" in says()


# ------------------------------------------------------------------------------------------------------------ CLI ----
def test_cli_key_is_parsed_and_refused():
    from slnlp import cli
    assert cli.gloss_structure_options(None) is None and "gloss_structure" in cli.DICT_ARGS
    assert cli.gloss_structure_options({}) == {"metric": "unit", "max_len": None, "top": 50}
    assert cli.gloss_structure_options({"metric": "phono", "top": 5}) == {"metric": "phono", "max_len": None, "top": 5}
    assert cli.gloss_structure_options({"max_len": 320})["max_len"] == 320
    for bad, says in (([1], "expected a dict"), ({"radius": 1}, "unknown keys"), ({"metric": "field"}, "metric="), ({"max_len": 64}, "max_len=64"),
                      ({"max_len": 513}, "max_len=513"), ({"metric": "phono", "max_len": 128}, "limited to 64 frames"), ({"top": -1}, "top=-1"),
                      ({"top": True}, "top=True"), ({"top": 2.0}, "top=2.0")):
        with pytest.raises(ValueError, match=f"gloss_structure.*{says}"):
            cli.gloss_structure_options(bad)
    X, L, y = dup_groups_ref.planted_rows()
    from slnlp.data import TokenDataset
    with pytest.raises(ValueError, match="gloss_structure: needs dataset_args.fields"):      # before anything touches a device
        cli.save_gloss_structure(TokenDataset(X, L, y), cli.gloss_structure_options({"metric": "phono"}), {}, "cuda:0", "/nonexistent")
