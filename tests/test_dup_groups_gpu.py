"""GPU: near-duplicate groups on the device -- ``slnlp_dup_groups_begin`` / ``_link`` / ``_finish`` through ``slnlp.ops`` and
``slnlp.duplicate_groups`` against the numpy restatement (tests/dup_groups_ref.py: the metrics' own restatements for the distances, a
plain union-find for the components).  ``group``, ``degree`` and the head are integers and EQUAL the restatement's: no tolerance
anywhere."""
import functools
import warnings

import numpy as np
import pytest
import torch

import dup_groups_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 257]                              # the wave edge and the 256-thread block edge
RADII = [0, 1, 2, 3]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dataset(X, L, y=None):
    from slnlp.data import TokenDataset
    return TokenDataset(X, L, np.zeros(len(L), dtype=np.int64) if y is None else y)


@functools.lru_cache(maxsize=None)
def random_case():
    """The 257 random rows and their unit-cost distances by the restatement, formed once and shared (nobody writes to them)"""
    X, L = ref.random_rows()
    dist, none = ref.distances(X, L)
    return X, L, dist, none


@functools.lru_cache(maxsize=None)
def random_want(n, radius):
    X, L, dist, none = random_case()
    return ref.groups(dist[:n, :n], none, radius)


def _same(got, want, what=""):
    assert got["group"].dtype == np.int32 and got["degree"].dtype == np.int32 and got["head"].dtype == np.int64
    assert np.array_equal(got["head"], want["head"]), (what, got["head"], want["head"])
    assert np.array_equal(got["degree"], want["degree"]), what
    assert np.array_equal(got["group"], want["group"]), what


def _link_all(dist, radius, chunks=None):
    """begin, link (the matrix uploaded, in ``chunks`` of query rows: default one), finish, download -- all on the current stream"""
    from slnlp import ops
    N = dist.shape[0]
    buf = ops.dup_groups_buffers(N, "cuda")
    for a, b in chunks or [(0, N)]:
        ops.dup_groups_link(_dev(dist[a:b]), a, radius, buf)
    ops.dup_groups_finish(buf)
    return {k: v.copy() for k, v in ops.dup_groups_download(buf).items()}


@pytest.mark.parametrize("n", SIZES)
def test_ops_equal_the_restatement_on_random_rows(n):
    X, L, dist, none = random_case()
    for radius in RADII:
        _same(_link_all(dist[:n, :n], radius), random_want(n, radius), f"N={n} radius={radius}")
    if n == 257:                                             # the chunks in any order, a short one among them; an odd start: unaligned rows
        want = random_want(n, 1)
        _same(_link_all(dist, 1, [(200, 257), (0, 100), (100, 101), (101, 200)]), want, "chunks out of order")
        wide = np.where(dist == none, 65535, dist).astype(np.uint16)
        _same(_link_all(wide, 1, [(0, 129), (129, 257)]), want, "the same distances as uint16")


@pytest.mark.parametrize("n", SIZES)
def test_duplicate_groups_equals_the_restatement_on_random_rows(n):
    import slnlp
    X, L, dist, none = random_case()
    y = (np.arange(n) % 3).astype(np.int64)
    for radius in RADII:
        want = random_want(n, radius)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # a generous radius chains: warned about, tested below
            got = slnlp.duplicate_groups(_dataset(X[:n], L[:n], y), radius)
        assert got["groups"].dtype == np.int64 and np.array_equal(got["groups"], want["group"]) and np.array_equal(got["degree"], want["degree"])
        sizes = np.bincount(want["group"], minlength=n)
        sizes = sizes[sizes > 0]
        assert (got["n_groups"], got["pairs"], got["flagged"]) == tuple(int(v) for v in want["head"][:3])
        assert np.array_equal(got["sizes"], sizes) and got["largest"] == sizes.max() and got["rows_in_groups"] == sizes[sizes > 1].sum()
        mixed = sum(len(set(y[want["group"] == r].tolist())) > 1 for r in np.unique(want["group"]))
        assert got["mixed_label_groups"] == mixed and (got["radius"], got["max_distance"], got["rows"]) == (radius, 64, n)


def test_a_chain_grows_the_deepest_trees():
    import slnlp
    X, L = ref.chain_rows(64)
    dist, none = ref.distances(X, L)
    assert dist[5, 9] == 4 and dist[63, 0] == 63
    one = _link_all(dist, 1)
    _same(one, ref.groups(dist, none, 1), "chain, radius 1")
    assert not one["group"].any() and one["head"][:2].tolist() == [1, 63]
    none0 = _link_all(dist, 0)
    _same(none0, ref.groups(dist, none, 0), "chain, radius 0")
    assert none0["group"].tolist() == list(range(64)) and none0["head"][:2].tolist() == [64, 0]
    with pytest.warns(RuntimeWarning, match="largest group holds 64 of 64"):
        got = slnlp.duplicate_groups(_dataset(X, L), 1)
    assert not got["groups"].any() and got["largest"] == 64 and got["pairs"] == 63
    X, L = ref.chain_rows(301)                               # the uint16 path: rows of up to 300 frames
    steps = np.abs(np.arange(301)[:, None] - np.arange(301)[None, :]).astype(np.uint16)      # d(i, j) = |i - j|, stated outright
    assert np.array_equal(steps[:40, :40], ref.distances(X[:40], L[:40], max_len=320)[0])
    want = ref.groups(steps, 65535, 1)
    assert not want["group"].any() and want["head"][:2].tolist() == [1, 300]
    with pytest.warns(RuntimeWarning, match="largest group"):
        got = slnlp.duplicate_groups(_dataset(X, L), 1, max_len=320)
    assert np.array_equal(got["groups"], want["group"]) and np.array_equal(got["degree"], want["degree"]) and got["pairs"] == 300
    assert got["max_distance"] == 320 and got["flagged"] == 0
    apart = slnlp.duplicate_groups(_dataset(X, L), 0, max_len=320)
    assert apart["groups"].tolist() == list(range(301)) and apart["pairs"] == 0 and apart["n_groups"] == 301


def test_identical_rows_are_one_group_under_full_contention():
    import slnlp
    X, L = np.full((300, 9), 7, dtype=np.int64), np.full(300, 9, dtype=np.int64)
    with pytest.warns(RuntimeWarning):
        got = slnlp.duplicate_groups(_dataset(X, L), 0)
    assert not got["groups"].any() and (got["degree"] == 299).all()
    assert (got["n_groups"], got["largest"], got["pairs"], got["rows_in_groups"], got["flagged"]) == (1, 300, 300 * 299 // 2, 300, 0)
    _same(_link_all(np.zeros((300, 300), dtype=np.uint8), 0), ref.groups(np.zeros((300, 300), dtype=np.uint8), 255, 0), "300 identical rows")


def test_unusable_rows_are_flagged_singletons():
    import slnlp
    rs = np.random.RandomState(2)
    X = rs.randint(2, 5, size=(40, 80)).astype(np.int64)     # stride 80: a row of 65 frames fits its row and is refused all the same
    L = rs.randint(0, 6, size=40).astype(np.int64)
    for i in (0, 7, 8, 39):
        X[i], L[i] = X[0], 65                                # identical to each other
    want = ref.duplicate_groups(X, L, 1)
    assert want["head"][2] == 4 and not want["degree"][[0, 7, 8, 39]].any() and want["group"][[0, 7, 8, 39]].tolist() == [0, 7, 8, 39]
    got = slnlp.duplicate_groups(_dataset(X, L), 1)
    assert np.array_equal(got["groups"], want["group"]) and np.array_equal(got["degree"], want["degree"])
    assert (got["flagged"], got["n_groups"], got["pairs"]) == (4, int(want["head"][0]), int(want["head"][1]))


def test_chunks_give_the_bytes_of_one_chunk():
    import slnlp
    from slnlp.edit_knn import query_chunks
    X, L, dist, none = random_case()
    ds = _dataset(X, L)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        whole = slnlp.duplicate_groups(ds, 2)
        chunks = query_chunks(257, 257, 60 * 257)
        assert len(chunks) == 5 and chunks[-1] == (240, 257)     # several chunks, a short last one
        parts = slnlp.duplicate_groups(ds, 2, cap=60 * 257)
        single = slnlp.duplicate_groups(ds, 2, cap=1)            # a row a chunk
        long_parts = slnlp.duplicate_groups(ds, 2, max_len=65, cap=2 * 60 * 257)
    for other in (parts, single, long_parts):
        for k in ("groups", "degree", "sizes"):
            assert other[k].tobytes() == whole[k].tobytes(), k
        assert all(other[k] == whole[k] for k in ("n_groups", "pairs", "flagged", "largest", "rows_in_groups"))
    assert np.array_equal(whole["groups"], random_want(257, 2)["group"])


@pytest.mark.parametrize("metric", ["long", "field", "field_gap", "weighted"])
def test_every_metric_equals_its_own_restatement(metric):
    import slnlp
    rs = np.random.RandomState(11)
    n = 130
    if metric == "long":
        X, L = ref.random_rows(n=n, S=128, tokens=3, seed=5)
        L[:40] = rs.randint(0, 6, size=40)                   # short rows: duplicates; long rows: the multi-word recurrence
        L[40:44] = [128, 127, 65, 64]
        X[41, :127] = X[40, :127]                            # rows 40 and 41 differ by one trailing frame
        kw, radius, bound = dict(max_len=128), 2, 128
    else:
        X, L = ref.random_rows(n=n, S=9, tokens=27, seed=6)
        L[:] = rs.randint(0, 5, size=n)
        codes = np.stack([np.arange(30) // 9, np.arange(30) // 3 % 3, np.arange(30) % 3], axis=1).astype(np.int64)      # F = 3; tokens 2..28
        kw = {"field": dict(field_codes=codes), "field_gap": dict(field_codes=codes, gap=2),
              "weighted": dict(field_codes=codes, field_weights=[2, 0, 1], gap=2)}[metric]
        radius, bound = 2, 64 * 3
    want = ref.duplicate_groups(X, L, radius, **kw)
    assert 1 < want["head"][0] < n and want["head"][1] > 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = slnlp.duplicate_groups(_dataset(X, L), radius, cap=2 * 50 * n, **kw)      # three chunks of 50, 50 and 30 rows
    assert np.array_equal(got["groups"], want["group"]) and np.array_equal(got["degree"], want["degree"])
    assert (got["n_groups"], got["pairs"], got["flagged"]) == tuple(int(v) for v in want["head"][:3]) and got["max_distance"] == bound
    print(f"{metric}: {got['n_groups']} groups of {n} rows, {got['pairs']} pairs, largest {got['largest']}")


def test_the_same_bytes_on_two_runs_and_two_streams():
    X, L, dist, none = random_case()
    first = _link_all(dist, 2)
    again = _link_all(dist, 2)
    others = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            others.append(_link_all(dist, 2, [(0, 100), (100, 257)]))
        stream.synchronize()
    for other in (again, *others):
        for k in ("head", "group", "degree"):
            assert other[k].tobytes() == first[k].tobytes(), k
    _same(first, random_want(257, 2))


def test_ops_refuse_what_the_library_would():
    from slnlp import ops
    buf = ops.dup_groups_buffers(8, "cuda")
    assert buf["shape"] == (8,) and buf["parent"].dtype == torch.int32 and buf["head"].dtype == torch.int64
    torch.cuda.synchronize()
    assert buf["parent"].cpu().tolist() == list(range(8)) and not buf["degree"].cpu().any() and not buf["head"].cpu().any()
    good = torch.zeros(2, 8, dtype=torch.uint8, device="cuda")
    for bad, says in ((good[:, :7], "dist must be"), (good.int(), "dist must be"), (good.t()[:8, :2], "dist must be"), (good.cpu(), "dist must be")):
        with pytest.raises(ValueError, match=says):
            ops.dup_groups_link(bad, 0, 0, buf)
    with pytest.raises(ValueError, match="radius=255"):
        ops.dup_groups_link(good, 0, 255, buf)
    with pytest.raises(ValueError, match="q0=8"):
        ops.dup_groups_link(good, 8, 0, buf)
    with pytest.raises(RuntimeError, match="q0=7"):                              # the library's own check: q0 + nq > N
        ops.dup_groups_link(good, 7, 0, buf)
    with pytest.raises(ValueError, match="buf must be"):
        ops.dup_groups_finish({"shape": (8, 2)})
    with pytest.raises(ValueError, match="N=0"):
        ops.dup_groups_buffers(0, "cuda")
