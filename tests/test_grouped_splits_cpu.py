"""CPU: leak-free splits -- the numpy restatement of the grouping (tests/dup_groups_ref.py) against scipy's connected components,
groups that travel with a ``TokenDataset``, every splitter honouring them (``split``, ``_train_split``, ``grid.build_tasks``,
``cross_fit``'s folds), the CLI key, and the argument checks of the three ``slnlp_dup_groups_*`` entry points, which return codes
before they touch a device.  Everything compared is an integer: every comparison is exact."""
import ctypes as C
import warnings

import numpy as np
import pytest

import dup_groups_ref as ref


# ---------------------------------------------------------------------------------------------------- restatement ----
@pytest.fixture(scope="module")
def random_case():
    X, L = ref.random_rows()
    dist, none = ref.distances(X, L)
    return X, L, dist, none


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_restatement_agrees_with_scipy_connected_components(random_case, radius):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    X, L, dist, none = random_case
    assert dist.shape == (257, 257) and np.array_equal(dist, dist.T)
    got = ref.groups(dist, none, radius)
    A = dist <= radius
    np.fill_diagonal(A, False)
    n, label = connected_components(csr_matrix(A), directed=False)
    first = np.full(n, len(label), dtype=np.int64)           # the lowest row index of every scipy component
    np.minimum.at(first, label, np.arange(len(label)))
    assert np.array_equal(got["group"], first[label])
    assert got["head"][0] == n and got["head"][1] == int(A.sum()) // 2 and got["head"][2] == 0 and not got["head"][3:4].any()
    assert np.array_equal(got["degree"], A.sum(1))
    sizes = np.bincount(label)
    print(f"radius {radius}: {n} groups, largest {sizes.max()}, {int(A.sum()) // 2} pairs")
    assert 1 < n < 257 and sizes.max() > 1                   # the rows hold duplicates, and the radius has not swallowed them


def test_restatement_keeps_unusable_rows_apart():
    X = np.full((5, 80), 3, dtype=np.int64)
    L = np.array([65, 4, 65, 4, 5], dtype=np.int64)          # rows 0 and 2 are beyond 64 frames and identical
    got = ref.duplicate_groups(X, L, 0)
    assert got["group"].tolist() == [0, 1, 2, 1, 4] and got["degree"].tolist() == [0, 1, 0, 1, 0]
    assert got["head"].tolist() == [4, 1, 2, 0, 2, 0, 0, 0]
    chain = ref.duplicate_groups(*ref.chain_rows(20), 1)
    assert not chain["group"].any() and chain["degree"].tolist() == [1] + [2] * 18 + [1] and chain["head"][:2].tolist() == [1, 19]
    assert ref.duplicate_groups(*ref.chain_rows(20), 0)["group"].tolist() == list(range(20))


# ----------------------------------------------------------------------------------------------- groups on a dataset ----
def planted(groups=True, alter=False):
    """The planted 300-row set (rows 100..159 copies of rows 0..59) and its exact-duplicate groups by the restatement"""
    from slnlp.data import TokenDataset
    X, L, y = ref.planted_rows(alter=alter)
    ds = TokenDataset(X, L, y)
    g = ref.duplicate_groups(X, L, 1 if alter else 0)["group"]
    assert len(np.unique(g)) == 240 and np.array_equal(g[100:160], np.arange(60))
    return (ds.with_groups(g) if groups else ds), g


def test_token_dataset_carries_groups_through_slicing():
    from slnlp.balance import balance_dataset
    from slnlp.data import TokenDataset
    ds, g = planted()
    plain, _ = planted(groups=False)
    assert plain.groups is None and plain[np.arange(5)].groups is None and plain.truncated(7).groups is None
    assert ds.groups.dtype == np.int64 and np.array_equal(ds.groups, g) and ds.ids is not None
    idx = np.array([150, 3, 299, 100])
    assert np.array_equal(ds[idx].groups, g[idx]) and np.array_equal(ds[idx].ids, plain[idx].ids)
    assert np.array_equal(ds[10:20].groups, g[10:20]) and np.array_equal(ds.truncated(120).groups, g[:120])
    assert np.array_equal(ds[(idx, Ellipsis)].groups, g[idx])                    # sklearn's _array_indexing
    assert ds[5] == plain[5]                                                     # an item is what it was
    assert np.array_equal(ds.with_groups({"groups": g, "n_groups": 240}).groups, g) and ds.with_groups(None).groups is None
    assert np.array_equal(TokenDataset(ds.ids, ds.lengths, ds.y, None, None).ids, ds.ids)      # the positional signature stands
    for bad in (g[:-1], g.astype(np.float64), g.reshape(1, -1), {"sizes": g}, "rows"):
        with pytest.raises(ValueError, match="groups"):
            plain.with_groups(bad)
    both = balance_dataset(ds, 1)                                                # an over-sampled row keeps its original's group
    assert both.groups is not None and len(both.groups) == len(both)
    where = {tuple(r.tolist()) + (int(l),): int(k) for r, l, k in zip(ds.ids, ds.lengths, ds.groups)}
    assert all(where[tuple(r.tolist()) + (int(l),)] == int(k) for r, l, k in zip(both.ids, both.lengths, both.groups))


@pytest.mark.parametrize("seed", [1, 2, 7])
def test_split_with_groups_keeps_every_group_on_one_side(seed):
    import torch
    ds, g = planted()
    plain, _ = planted(groups=False)
    n_test = int(round(300 * 0.2))
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(seed)).numpy()
    test0, train0 = plain.split(0.2, seed)                                       # groups=None: today's indices
    assert np.array_equal(test0.ids, plain.ids[perm[:n_test]]) and np.array_equal(train0.ids, plain.ids[perm[n_test:]])
    assert test0.groups is None and train0.groups is None
    single = plain.with_groups(np.arange(300)[::-1].copy())                      # all-singleton groups: the ungrouped split exactly
    test1, train1 = single.split(0.2, seed)
    assert np.array_equal(test1.ids, test0.ids) and np.array_equal(train1.ids, train0.ids) and np.array_equal(test1.y, test0.y)
    assert np.array_equal(test1.groups, single.groups[perm[:n_test]])
    test, train = ds.split(0.2, seed)
    assert len(test) + len(train) == 300 and not set(test.groups.tolist()) & set(train.groups.tolist())
    largest = int(np.bincount(g).max())
    assert n_test <= len(test) < n_test + largest
    key = lambda d: sorted(tuple(r.tolist()) + (int(l), int(c)) for r, l, c in zip(d.ids, d.lengths, d.y))
    assert sorted(key(test) + key(train)) == key(ds)                             # a partition of the rows
    again = ds.split(0.2, seed)
    assert np.array_equal(again[0].ids, test.ids) and np.array_equal(again[1].ids, train.ids)
    crossing = len(set(g[perm[:n_test]].tolist()) & set(g[perm[n_test:]].tolist()))
    print(f"seed {seed}: the ungrouped split cuts {crossing} groups; the grouped test side holds {len(test)} rows")
    assert crossing > 0                                                          # the ungrouped split does leak here


def test_split_by_count_and_an_oversized_group():
    from slnlp.data import TokenDataset, grouped_split
    test, train = grouped_split(np.array([4, 0, 1, 2, 3, 5]), np.array([0, 0, 0, 3, 3, 5]), 2)
    assert test.tolist() == [4, 3] and train.tolist() == [0, 1, 2, 5]            # row 4 brings its group {3, 4}; group 0 arrives when test is full
    test, train = grouped_split(np.array([0, 1, 2, 3]), np.zeros(4, dtype=np.int64), 1)
    assert test.tolist() == [0, 1, 2, 3] and train.tolist() == []                # one group: it goes where its first row goes
    ds = TokenDataset(np.zeros((6, 2)), np.ones(6), np.arange(6)).with_groups([0, 0, 2, 2, 4, 4])
    a, b = ds.split(2, 3)
    assert len(a) == 2 and len(b) == 4 and not set(a.groups.tolist()) & set(b.groups.tolist())


# ---------------------------------------------------------------------------------------------------------- folds ----
def _whole(folds, g, n):
    held = np.concatenate([h for _, h in folds])
    assert sorted(held.tolist()) == list(range(n))                               # the held-out sides partition the rows
    for train, held_out in folds:
        assert sorted(np.concatenate([train, held_out]).tolist()) == list(range(n))
        assert not set(g[train].tolist()) & set(g[held_out].tolist())


@pytest.mark.parametrize("cv", [3, 5])
def test_grid_and_cross_fit_folds_keep_groups_whole(cv):
    from slnlp import grid
    from slnlp.out_of_fold import cross_fit_folds
    ds, g = planted()
    plain, _ = planted(groups=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                           # the planted set needs no fallback and draws no warning
        cands, folds, tasks, order = grid.build_tasks({"lr": [0.1, 0.2]}, ds.y, cv, groups=ds.groups)
        again = grid.build_tasks({"lr": [0.1, 0.2]}, ds.y, cv, groups=ds.groups)[1]
        oof = cross_fit_folds(ds, cv)
    _whole(folds, g, 300)
    print(f"cv {cv}: grouped fold sizes {[len(h) for _, h in folds]}")
    # the exact sizes depend on how the glosses fall on the rows; with groups of at most two rows and 25 rows a gloss a fold
    # stays within the largest group of 300 / cv (sklearn 1.7's StratifiedGroupKFold gave 101 / 100 / 99 and 60 / 60 / 61 / 60 / 59
    # on another draw of the labels)
    assert len(folds) == cv and all(abs(len(h) - 300 / cv) <= 2 for _, h in folds)
    assert len(tasks) == 2 * cv and sorted(order) == list(range(2 * cv))
    for (a, b), (c, d), (e, f) in zip(folds, again, oof):
        assert np.array_equal(a, c) and np.array_equal(b, d) and np.array_equal(a, e) and np.array_equal(b, f)
    from sklearn.model_selection import StratifiedKFold                          # without groups: the stratified folds, unchanged
    want = list(StratifiedKFold(n_splits=cv).split(np.zeros(300), plain.y))
    for got in (grid.build_tasks({"lr": [0.1]}, plain.y, cv)[1], cross_fit_folds(plain, cv)):
        assert all(np.array_equal(a, c) and np.array_equal(b, d) for (a, b), (c, d) in zip(got, want))
    cut = sum(bool(set(g[a].tolist()) & set(g[b].tolist())) for a, b in want)
    assert cut >= 1                                                              # the stratified folds do cut groups here
    units = grid.build_units(cands, folds, tasks, order, lockstep=4)             # fits of unequal folds land in different units
    assert sorted(t for u in units for t in u) == list(range(2 * cv))
    assert all(len({(len(folds[tasks[t][1]][0]), len(folds[tasks[t][1]][1])) for t in u}) == 1 for u in units)


def test_train_split_keeps_groups_whole_and_names_what_it_cannot_do():
    from slnlp.net import NeuralNetClassifier
    ds, g = planted()
    plain, _ = planted(groups=False)
    net = NeuralNetClassifier(module="model.Transformer")
    assert net.train_split == 5
    tr, va = net._train_split(ds)
    tr2, va2 = net._train_split(ds)
    assert np.array_equal(tr, tr2) and np.array_equal(va, va2)
    assert sorted(np.concatenate([tr, va]).tolist()) == list(range(300)) and not set(g[tr].tolist()) & set(g[va].tolist())
    assert 55 <= len(va) <= 65
    from sklearn.model_selection import StratifiedKFold                          # without groups: the first stratified fold, as ever
    tr0, va0 = next(iter(StratifiedKFold(n_splits=5).split(np.arange(300), plain.y)))
    got = net._train_split(plain)
    assert np.array_equal(got[0], tr0) and np.array_equal(got[1], va0)
    sub = ds[tr]                                                                 # a fold of a grouped dataset splits on its own groups
    a, b = net._train_split(sub)
    assert not set(sub.groups[a].tolist()) & set(sub.groups[b].tolist())
    rare = plain.with_groups(g)
    rare.y[:] = np.arange(300) + 2                                               # no class has five members: the GroupKFold fall-back
    a, b = net._train_split(rare)
    assert not set(g[a].tolist()) & set(g[b].tolist()) and len(a) + len(b) == 300
    few = plain.with_groups(np.arange(300) % 3)
    with pytest.raises(ValueError, match=r"NeuralNetClassifier: train_split=5 folds over 3 groups .*300 rows"):
        net._train_split(few)
    net.set_params(train_split=None)
    assert net._train_split(few)[1] is None


def test_fewer_groups_than_folds_raises_the_named_error():
    from slnlp import grid
    from slnlp.out_of_fold import cross_fit_folds
    plain, _ = planted(groups=False)
    few = plain.with_groups(np.arange(300) % 2)
    with pytest.raises(ValueError, match=r"build_tasks: cv=3 folds over 2 groups"):
        grid.build_tasks({"lr": [0.1]}, few.y, 3, groups=few.groups)
    with pytest.raises(ValueError, match=r"cross_fit: cv=3 folds over 2 groups"):
        cross_fit_folds(few, 3)
    with pytest.raises(ValueError, match="groups must be an integer array"):
        grid.build_tasks({"lr": [0.1]}, few.y, 3, groups=few.groups[:-1])
    assert len(grid.build_tasks({"lr": [0.1]}, few.y, 2, groups=few.groups)[1]) == 2


# ------------------------------------------------------------------------------------------------------------ CLI ----
def test_cli_key_is_parsed_and_refused():
    from slnlp import cli
    assert cli.grouped_splits_options(None) is None and "grouped_splits" in cli.DICT_ARGS
    assert cli.grouped_splits_options({}) == {"radius": 0, "metric": "unit", "max_len": None}
    assert cli.grouped_splits_options({"radius": 64})["radius"] == 64
    assert cli.grouped_splits_options({"radius": 200, "max_len": 320}) == {"radius": 200, "metric": "unit", "max_len": 320}
    assert cli.grouped_splits_options({"metric": "phono", "radius": 1024})["metric"] == "phono"
    for bad, says in (([1], "expected a dict"), ({"k": 1}, "unknown keys"), ({"metric": "field"}, "metric="), ({"radius": 65}, "radius=65"),
                      ({"radius": -1}, "radius=-1"), ({"radius": True}, "radius=True"), ({"radius": 1.0}, "radius=1.0"),
                      ({"max_len": 64}, "max_len=64"), ({"max_len": 513}, "max_len=513"), ({"radius": 321, "max_len": 320}, "radius=321"),
                      ({"metric": "phono", "max_len": 128}, "limited to 64 frames"), ({"metric": "phono", "radius": 1025}, "radius=1025")):
        with pytest.raises(ValueError, match=f"grouped_splits.*{says}"):
            cli.grouped_splits_options(bad)
    ds, _ = planted(groups=False)
    with pytest.raises(ValueError, match="grouped_splits: needs dataset_args.fields"):      # before anything touches a device
        cli.apply_grouped_splits(ds, cli.grouped_splits_options({"metric": "phono"}), {}, "cuda:0")


def test_public_function_checks_its_arguments_before_the_device():
    import slnlp
    from slnlp import dup_groups
    assert slnlp.duplicate_groups is dup_groups.duplicate_groups and "duplicate_groups" in slnlp.__all__
    ds, _ = planted(groups=False)
    codes = np.arange(50 * 3).reshape(50, 3) % 5
    for kw, err, says in ((dict(radius=65), ValueError, "radius=65"), (dict(radius=129, max_len=128), ValueError, "radius=129"),
                          (dict(max_len=64), ValueError, "max_len=64"), (dict(max_len=128, field_codes=codes), ValueError, "limited to 64 frames"),
                          (dict(gap=1), ValueError, "without field_codes"), (dict(field_weights=[1, 1, 1]), ValueError, "without field_codes"),
                          (dict(field_codes=codes, radius=193), ValueError, "radius=193"), (dict(field_codes=codes, gap=4), ValueError, "gap=4"),
                          (dict(field_codes=codes, field_weights=[1, 2]), ValueError, "field_weights"), (dict(cap=0), ValueError, "cap=0"),
                          (dict(device="cpu"), ValueError, "cuda device")):
        with pytest.raises(err, match=says):
            slnlp.duplicate_groups(ds, **kw)
    with pytest.raises(TypeError, match="TokenDataset"):
        slnlp.duplicate_groups(np.zeros((3, 3)))
    rep = dup_groups.groups_report(np.array([0, 0, 2, 0]), np.array([2, 2, 0, 2]), np.array([2, 3, 0, 0, 6, 0, 0, 0]), np.array([5, 5, 6, 7]), 1, 64)
    assert rep["sizes"].tolist() == [3, 1] and (rep["n_groups"], rep["largest"], rep["rows_in_groups"], rep["pairs"]) == (2, 3, 3, 3)
    assert rep["mixed_label_groups"] == 1 and rep["flagged"] == 0 and rep["groups"].dtype == np.int64 and rep["max_distance"] == 64


# ------------------------------------------------------------------------------------------------------------ ABI ----
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    return _lib.load()


def test_entry_points_validate_before_they_touch_a_device(lib):
    """slnlp_dup_groups_begin / _link / _finish check pointers, counts, width, radius, alignment and overlaps first: codes and
    messages, no launch, no GPU needed."""
    INVALID = 1                                                                  # SLNLP_ERR_INVALID_ARG
    mem = (C.c_int64 * 4096)()
    base = C.cast(mem, C.c_void_p).value                                         # non-null addresses: nothing below gets as far as reading them
    dist, parent, degree, group, head = base, base + 8192, base + 12288, base + 16384, base + 20480
    says = lambda: lib.slnlp_last_error().decode()
    N = 64

    def begin(parent=parent, degree=degree, N=N, head=head):
        return lib.slnlp_dup_groups_begin(parent, degree, N, head, None)

    def link(dist=dist, width=1, nq=8, N=N, q0=0, radius=1, parent=parent, degree=degree, head=head):
        return lib.slnlp_dup_groups_link(dist, width, nq, N, q0, radius, parent, degree, head, None)

    def finish(parent=parent, N=N, group=group, head=head):
        return lib.slnlp_dup_groups_finish(parent, N, group, head, None)

    for call in (begin, link, finish):
        for name in ("parent", "head"):
            assert call(**{name: None}) == INVALID and "null pointer" in says()
        for bad in (0, -1, 2 ** 30 + 1):
            assert call(N=bad) == INVALID and "outside 1..1073741824" in says()
        assert call(head=head + 4) == INVALID and "misaligned" in says()
        assert call(parent=parent + 2) == INVALID and "misaligned" in says()
    assert begin(degree=None) == INVALID and "dup_groups_begin: null pointer" in says()
    assert begin(degree=parent + 4 * (N - 1)) == INVALID and "outputs parent and degree overlap" in says()
    assert begin(head=parent + 8) == INVALID and "overlap" in says()
    assert link(dist=None) == INVALID and "dup_groups_link: null pointer" in says()
    for bad in (0, 3, 4, -1):
        assert link(width=bad) == INVALID and f"width={bad}" in says()
    for bad in (0, -3, 2 ** 30 + 1):
        assert link(nq=bad) == INVALID and "nq=" in says()
    assert link(nq=8, q0=57) == INVALID and "q0=57" in says()                    # q0 + nq > N
    assert link(q0=-1) == INVALID and "q0=-1" in says()
    assert link(nq=65) == INVALID
    assert link(nq=2 ** 16, N=2 ** 16, parent=base + (1 << 40), degree=base + (2 << 40), head=base + (3 << 40)) == INVALID and "pairs" in says()
    for width, bad in ((1, 255), (1, -1), (2, 65535), (2, -1), (1, 300)):
        assert link(width=width, radius=bad) == INVALID and f"radius={bad}" in says()
    assert link(width=2, dist=dist + 1) == INVALID and "misaligned" in says()
    assert link(degree=degree + 1) == INVALID and "misaligned" in says()
    assert link(dist=parent - 8 * N + 4) == INVALID and "output parent overlaps input dist" in says()
    assert link(width=2, nq=8, dist=parent - 2 * 8 * N + 2) == INVALID and "output parent overlaps input dist" in says()
    assert link(head=dist + 8) == INVALID and "output head overlaps input dist" in says()
    assert finish(group=None) == INVALID and "dup_groups_finish: null pointer" in says()
    assert finish(group=parent + 4) == INVALID and "output group overlaps input parent" in says()
    assert finish(head=parent) == INVALID and "output head overlaps input parent" in says()
    assert finish(group=group + 1) == INVALID and "misaligned" in says()
