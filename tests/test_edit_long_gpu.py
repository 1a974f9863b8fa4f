"""GPU: edit-distance nearest neighbours of rows longer than 64 frames -- ``slnlp_edit_long_distances``, ``slnlp_edit_long_knn_rows``
and ``slnlp_edit_long_knn_logp`` (csrc/edit_long.hip: Myers' recurrence in its multi-word form) through ``slnlp.ops`` against the numpy
restatement (tests/edit_long_ref.py), then ``EditKNN(max_len=...)`` and ``split_audit(..., max_len=...)`` end to end.

The bounds are those of tests/test_edit_knn_gpu.py.  Distances, neighbours, the per-query rows and the head are integers and EQUAL
the restatement's.  The vote is formed in fp64 in the restatement's order of operations -- it is the same kernel as the 64-frame
search's, with another bound --; the device's exp and log may differ from numpy's by an fp64 ulp, which moves the float32 rounding
of log(p) by at most one unit: every finite entry lies within ONE float32 ulp (``np.spacing`` of the restatement's value) of the
restatement, NaN rows match exactly, and the arg-max equals the restatement's wherever its top-two gap exceeds that ulp.  Where
every row has at most 64 frames the long path and the 64-frame path agree value for value and bit for bit.

The inputs.  In every case the rows lie S + 3 tokens apart, and the padding and the tokens past a row's length are tokens of the
alphabet both sides draw from, so a read past L changes a distance.  Cases with at least 8 queries and 9 references carry a query
and a reference of lengths max_len + 1 and -1, an ``exclude`` list with -1 entries, and duplicated rows (distance 0, index ties)."""
import functools

import numpy as np
import pytest
import torch

import edit_long_ref as ref

pytestmark = pytest.mark.gpu

RADIUS = 50                                                  # within every case's max_len (the smallest is 65)
#         nq   nr    S  max_len k  alphabet
SHAPES = [(1, 1, 65, 65, 1, "small"),           # the smallest two-word query: one bit in the second word
          (5, 7, 128, 128, 3, "small"),         # lengths 0, 1, 127 and 128 on both sides: the top bit of word 1
          (8, 9, 129, 129, 5, "small"),         # 128 and 129; flagged rows, exclude, duplicates
          (9, 12, 512, 512, 5, "three"),        # the cap: 511 and 512, two identical rows of 512 tokens (bit 63 of word 7), 513 flagged
          (33, 40, 300, 300, 64, "one"),        # ONE token: every mask all ones, the carry ripples through every word; k at its cap
          (65, 257, 200, 200, 5, "wide"),       # more references than a block's threads, queries past a wave, 1, 2, 3 and 4 words
          (8, 9, 512, 512, 5, "distinct"),      # 512 distinct tokens in one query: the hash at half load, two positions a thread
          (33, 40, 130, 130, 5, "high"),        # tokens that differ only above bit 32: a 32-bit compare shows
          (16, 20, 128, 100, 5, "small")]       # max_len below the row: lengths 101..128 are refused although they fit
IDS = [f"{nq}x{nr}x{S}m{ml}k{k}{name}" for nq, nr, S, ml, k, name in SHAPES]
ALPHABETS = {"small": np.arange(2, 8), "wide": np.arange(2, 40), "three": np.arange(5, 8), "one": np.arange(9, 10),
             "distinct": np.arange(2, 4002), "high": (np.arange(1, 5, dtype=np.int64) << 33) + 7}      # 2^33 t + 7: equal in their low 32 bits


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _lengths(rs, n, S):
    """random ones, then S, 0, S - 1 and 1 in the last places (as far as n goes): the rows a case rewrites are the first six"""
    edge = np.array([S, 0, S - 1, 1], dtype=np.int64)[:n]
    return np.concatenate([rs.randint(0, S + 1, size=n - len(edge)), edge]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(index):
    """One shape's inputs and the restatement's outputs, formed once and shared (nobody writes to them)"""
    nq, nr, S, max_len, k, name = SHAPES[index]
    rs = np.random.RandomState(300 + index)
    alphabet = ALPHABETS[name]
    token = lambda m: rs.choice(alphabet, size=m, replace=name != "distinct")
    Xq, Lq = ref.make_rows(rs, nq, S, alphabet, _lengths(rs, nq, S), token)
    Xr, Lr = ref.make_rows(rs, nr, S, alphabet, _lengths(rs, nr, S), token)
    exclude = None
    if nq >= 8 and nr >= 9:
        full = min(S, max_len)
        Lr[0] = full                                         # max_len = 512: two identical rows of 512 tokens, bit 63 of word 7 all the way
        Xr[0, :full] = token(full)
        Xr[5], Lr[5] = Xr[0], Lr[0]                          # a duplicated reference, and a query that equals both
        Xq[0], Lq[0] = Xr[0], Lr[0]
        Xq[4, :min(Lq[4], Lr[6])] = Xr[6, :min(Lq[4], Lr[6])]
        Lq[1], Lq[3], Lr[2], Lr[4] = max_len + 1, -1, max_len + 1, -1     # max_len + 1 fits the row of S + 3 tokens: refused all the same
        exclude = np.where(rs.rand(nq) < 0.5, -1, rs.randint(0, nr, size=nq)).astype(np.int64)
        exclude[0], exclude[2] = 0, -1                       # query 0 skips its twin 0 and finds the copy 5
    if name == "wide":                                       # queries of 1, 2, 3 and 4 words in one launch, at the words' edges
        Lq[6:14] = [64, 65, 128, 129, 192, 193, 7, 100]
    dist = ref.distances(Xq[:, :S], Lq, Xr[:, :S], Lr, max_len)
    res = ref.knn_rows(dist, Lq, Lr, S, S, k, max_len, radius=RADIUS, exclude=exclude)
    return dict(nq=nq, nr=nr, S=S, max_len=max_len, k=k, Xq=Xq, Lq=Lq, Xr=Xr, Lr=Lr, exclude=exclude, dist=dist, res=res)


@functools.lru_cache(maxsize=None)
def far_case():
    """Every neighbour further than 255 edits away: queries of 500 to 512 frames over a wide alphabet, references of at most 100
    frames (rows of another width).  A matrix truncated to one byte, or a vote whose bound stayed at 64, shows as wrong log-probs."""
    rs = np.random.RandomState(77)
    alphabet = ALPHABETS["wide"]
    token = lambda m: rs.choice(alphabet, size=m)
    nq, nr, k = 6, 20, 5
    Xq, Lq = ref.make_rows(rs, nq, 512, alphabet, rs.randint(500, 513, size=nq), token)
    Xr, Lr = ref.make_rows(rs, nr, 100, alphabet, rs.randint(0, 101, size=nr), token)
    Lq[0], Lr[0] = 512, 100
    dist = ref.distances(Xq[:, :512], Lq, Xr[:, :100], Lr, 512)
    res = ref.knn_rows(dist, Lq, Lr, 512, 100, k, 512, radius=RADIUS)
    assert dist.min() > 255 and (res["nbr"][:, :, 0] > 255).all() and (res["rows"][:, 0] == k).all()
    return dict(nq=nq, nr=nr, S=512, max_len=512, k=k, Xq=Xq, Lq=Lq, Xr=Xr, Lr=Lr, exclude=None, dist=dist, res=res, Sr=100)


def _device_rows(c):
    """The rows as the device sees them: [n, S] views of tensors whose rows lie S + 3 apart"""
    return _dev(c["Xq"])[:, :c["S"]], _dev(c["Lq"]), _dev(c["Xr"])[:, :c.get("Sr", c["S"])], _dev(c["Lr"])


def _search(c, sl=slice(None)):
    from slnlp import ops
    Xq, Lq, Xr, Lr = _device_rows(c)
    ex = None if c["exclude"] is None else _dev(c["exclude"])[sl]
    return ops.edit_long_knn_rows(Xq[sl], Lq[sl], Xr, Lr, c["k"], max_len=c["max_len"], radius=RADIUS, exclude=ex)


def _same(got, want, what):
    wrong = np.argwhere(np.asarray(got) != np.asarray(want))
    assert got.shape == want.shape and wrong.size == 0, (f"{len(wrong)} of {want.size} {what} differ, first at {wrong[0]}: "
                                                         f"{got[tuple(wrong[0])]} != {want[tuple(wrong[0])]}")


# ---------------------------------------------------------------------------------------------------------- integers ----
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=IDS)
def test_distances_equal_restatement(index):
    from slnlp import ops
    c = case(index)
    got = ops.edit_long_distances(*_device_rows(c), max_len=c["max_len"]).cpu().numpy()
    assert got.dtype == np.uint16
    _same(got, c["dist"], "distances")


@pytest.mark.parametrize("index", range(len(SHAPES)), ids=IDS)
def test_neighbours_equal_restatement(index):
    from slnlp import ops
    c = case(index)
    got = ops.edit_knn_download(_search(c))
    want = c["res"]
    _same(got["rows"], want["rows"], "row entries")
    _same(got["nbr"], want["nbr"], "neighbour entries")
    _same(got["head"], want["head"], "head entries")
    if c["exclude"] is not None:                             # what the case was built to hold
        assert (want["rows"][[1, 3], 3] == 1).all() and (want["nbr"][[1, 3]] == -1).all() and tuple(want["nbr"][0, 0]) == (0, 5)
        if c["S"] == c["max_len"]:
            assert got["head"][0] == 2 and got["head"][1] == 2


def test_what_the_cases_were_built_to_hold():
    words = lambda c: set(((c["Lq"][(c["Lq"] > 0) & (c["Lq"] <= c["max_len"])] - 1) >> 6) + 1)
    assert case(0)["Lq"].tolist() == [65] and case(0)["dist"].shape == (1, 1)
    assert {0, 1, 127, 128} <= set(case(1)["Lq"]) and {0, 1, 127, 128} <= set(case(1)["Lr"])
    c = case(3)
    assert {511, 512} <= set(c["Lq"]) and c["dist"][0, 0] == 0 and c["dist"][0, 5] == 0 and c["Lq"][0] == 512 and c["Lq"][1] == 513
    c = case(4)                                              # one token: the distance is the length difference, ties dominate
    okq, okr = (c["Lq"] >= 0) & (c["Lq"] <= 300), (c["Lr"] >= 0) & (c["Lr"] <= 300)
    assert np.array_equal(c["dist"][okq][:, okr], np.abs(c["Lq"][okq][:, None] - c["Lr"][okr][None, :]))
    assert (c["res"]["rows"][okq, 0] >= 40 - 2 - 1).all()   # every usable reference but the excluded one: found < k = 64
    assert words(case(5)) == {1, 2, 3, 4} and case(5)["nr"] > 256
    c = case(6)
    assert len(set(c["Xq"][0, :512])) == 512 and c["Lq"][0] == 512
    c = case(8)                                              # lengths 101..128 fit the row of 131 tokens and are refused
    inside = lambda L: int(((L > 100) & (L <= 128)).sum())
    assert inside(c["Lq"]) >= 2 and inside(c["Lr"]) >= 2
    assert c["res"]["head"][0] == ((c["Lq"] < 0) | (c["Lq"] > 100)).sum() and c["res"]["head"][1] == ((c["Lr"] < 0) | (c["Lr"] > 100)).sum()


# ------------------------------------------------------------------------------------------------------------- votes ----
@pytest.mark.parametrize("weights", ["uniform", "distance"])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("which,V", [(2, 7), (5, 70), ("far", 5)], ids=["8x9x129", "65x257x200", "far"])
def test_votes_within_one_float32_ulp(which, V, normalize, weights):
    from slnlp import ops
    c = far_case() if which == "far" else case(which)
    rs = np.random.RandomState(7 + V)
    yr = rs.randint(0, V, size=c["nr"]).astype(np.int64)
    yr[1], yr[3] = -1, V                                     # labels outside the classes: skipped and counted
    prior = ref.prior_of(yr[(yr >= 0) & (yr < V)], V)
    tau, lam = 0.75, 0.5
    want, bad = ref.knn_logp(c["res"], c["Lq"], c["Lr"], yr, prior, c["max_len"], weights=weights, tau=tau, normalize=normalize, lam=lam)
    buf = _search(c)
    out = torch.full((c["nq"], V + 3), 7.0, dtype=torch.float32, device="cuda")          # padded rows: the padding stays
    ops.edit_long_knn_logp(buf, _dev(c["Lq"]), _dev(c["Lr"]), _dev(yr), _dev(prior), max_len=c["max_len"], weights=weights, tau=tau,
                           normalize=normalize, lam=lam, out=out[:, :V])
    full = out.cpu().numpy()
    got = full[:, :V]
    assert (full[:, V:] == 7.0).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want).all(axis=1).sum() == c["res"]["head"][0] == (0 if which == "far" else 2)
    fin = ~np.isnan(want)
    assert np.isfinite(want[fin]).all() and np.isfinite(got[fin]).all()
    ulp = np.spacing(np.abs(want[fin]))
    print(f"\n{(got[fin] != want[fin]).sum()} of {fin.sum()} entries differ from the restatement; largest {np.max(np.abs(got[fin] - want[fin]) / ulp):.2f} ulp")
    assert (np.abs(got[fin] - want[fin]) <= ulp).all()
    rows = fin.all(axis=1)
    top2 = np.sort(want[rows], axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > np.spacing(np.abs(top2[:, 1]))
    assert np.array_equal(got[rows].argmax(1)[clear], want[rows].argmax(1)[clear])
    assert int(ops.edit_knn_download(buf, neighbours=False)["head"][2]) == bad
    if which == "far" and (weights == "uniform" or normalize):   # the prior alone -- what a bound left at 64 gives -- is not the answer
        # (unnormalised distance weights exp(-d / 0.75) at d > 255 underflow to 0 in fp64: there the prior IS the vote)
        assert (np.abs(got - np.log(prior).astype(np.float32)[None, :]) > 1e-3).any(axis=1).all()


# --------------------------------------------------------------------------------------- agreement with the short path ----
def test_agrees_with_the_64_frame_path_where_both_apply():
    import slnlp
    from slnlp import ops
    from slnlp.data import synthetic_dataset
    rs = np.random.RandomState(11)
    alphabet = ALPHABETS["small"]
    token = lambda m: rs.choice(alphabet, size=m)
    Xq, Lq = ref.make_rows(rs, 33, 64, alphabet, _lengths(rs, 33, 64), token)
    Xr, Lr = ref.make_rows(rs, 40, 64, alphabet, _lengths(rs, 40, 64), token)
    rows = _dev(Xq)[:, :64], _dev(Lq), _dev(Xr)[:, :64], _dev(Lr)
    short, long = ops.edit_distances(*rows).cpu().numpy(), ops.edit_long_distances(*rows, max_len=512).cpu().numpy()
    assert short.max() <= 64
    _same(long.astype(np.int64), short.astype(np.int64), "distances")
    ds = synthetic_dataset(400, seq_len=12, src_vocab=64, n_labels=6, seed=5, min_len=3)
    train, test = ds[np.arange(300)], ds[np.arange(300, 400)]
    a = slnlp.EditKNN(k=5).fit(train)._forward_logp(test, lambda z, y: z.cpu().numpy())
    b = slnlp.EditKNN(k=5, max_len=512).fit(train)._forward_logp(test, lambda z, y: z.cpu().numpy())
    assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b) and np.isfinite(a).all()


# ------------------------------------------------------------------------------------------------------ equal bytes ----
def test_equal_bytes_across_runs():
    from slnlp import ops
    c = case(5)
    yr = _dev(np.random.RandomState(3).randint(0, 9, size=c["nr"]).astype(np.int64))
    prior = _dev(np.full(9, 1.0 / 9))

    def run():
        buf = _search(c)
        z = ops.edit_long_knn_logp(buf, _dev(c["Lq"]), _dev(c["Lr"]), yr, prior, max_len=c["max_len"])
        got = ops.edit_knn_download(buf)
        return got["rows"].copy(), got["nbr"].copy(), z.cpu().numpy()
    a, b = run(), run()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                            # another stream: the same bytes
        s = run()
    side.synchronize()
    for i in range(3):
        assert a[i].tobytes() == b[i].tobytes() == s[i].tobytes()


def test_library_refusals():
    """SLNLP_ERR_INVALID_ARG with the entry point's name, before anything is launched"""
    import ctypes as C
    from slnlp import _lib, ops
    c = case(1)
    Xq, Lq, Xr, Lr = _device_rows(c)
    whole = _dev(c["Xq"])
    Xq = whole[:, :128]
    for bad in (0, 513):
        with pytest.raises(RuntimeError, match=rf"code 1\): edit_long_distances: max_len={bad} outside 1..512"):
            ops.edit_long_distances(Xq, Lq, Xr, Lr, max_len=bad)
        with pytest.raises(RuntimeError, match=rf"code 1\): edit_long_knn_rows: max_len={bad} outside 1..512"):
            ops.edit_long_knn_rows(Xq, Lq, Xr, Lr, 2, max_len=bad)
    with pytest.raises(RuntimeError, match=r"code 1\): edit_long_knn_rows: radius=129 outside 0..max_len=128"):
        ops.edit_long_knn_rows(Xq, Lq, Xr, Lr, 2, max_len=128, radius=129)
    with pytest.raises(RuntimeError, match=r"code 1\): edit_long_knn_rows: scratch of 69 bytes is too small"):
        ops.edit_long_knn_rows(Xq, Lq, Xr, Lr, 2, max_len=128, scratch=torch.empty(2 * 5 * 7 - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match=r"code 1\): edit_long_distances: output dist overlaps input query"):
        ops.edit_long_distances(Xq, Lq, Xr, Lr, max_len=128, out=whole.view(torch.uint16).flatten()[:35].view(5, 7))
    buf = ops.edit_long_knn_rows(Xq, Lq, Xr, Lr, 2, max_len=128)
    with pytest.raises(RuntimeError, match=r"code 1\): edit_long_knn_logp: max_len=513 outside 1..512"):
        ops.edit_long_knn_logp(buf, Lq, Lr, Lr, _dev(np.full(3, 1 / 3)), max_len=513)
    with pytest.raises(RuntimeError, match="edit_long_knn_logp: output head overlaps input prior"):
        ops.edit_long_knn_logp(buf, Lq, Lr, Lr, buf["head"].view(torch.float64)[:4], max_len=128)
    # a misaligned dist: no uint16 tensor starts at an odd address, so this one call goes to the library itself
    lib, raw = _lib.load(), torch.empty(2 * 5 * 7 + 2, dtype=torch.uint8, device="cuda")
    rc = lib.slnlp_edit_long_distances(Xq.data_ptr(), Xq.stride(0), Lq.data_ptr(), 5, Xr.data_ptr(), Xr.stride(0), Lr.data_ptr(), 7, 128,
                                       raw.data_ptr() + 1, None)
    assert rc == 1 and b"edit_long_distances: misaligned pointer (dist: 2 bytes)" in lib.slnlp_last_error()
    assert lib.slnlp_edit_long_knn_scratch_bytes(5, 7) == 70 and lib.slnlp_edit_long_knn_scratch_bytes(0, 7) == -1
    assert b"edit_long_knn_scratch_bytes" in lib.slnlp_last_error()
    torch.cuda.synchronize()                                 # nothing was launched: nothing to fault


# ------------------------------------------------------------------------------------------------------ end to end ----
@pytest.fixture(scope="module")
def data():
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(300, seq_len=150, src_vocab=64, n_labels=6, seed=5, min_len=3)
    assert ds.lengths.max() > 128 and ds.lengths.max() <= 150
    return ds[np.arange(200)], ds[np.arange(200, 300)]


@pytest.fixture(scope="module")
def expected(data):
    """The restatement on the end-to-end data: distances, the 5 neighbours, EditKNN's default vote"""
    train, test = data
    V, S = len(train.vocab_y), train.ids.shape[1]
    dist = ref.distances(test.ids, test.lengths, train.ids, train.lengths, 192)
    res = ref.knn_rows(dist, test.lengths, train.lengths, S, S, 5, 192)
    logp, _ = ref.knn_logp(res, test.lengths, train.lengths, train.y, ref.prior_of(train.y, V), 192)
    return dict(dist=dist, res=res, logp=logp)


@pytest.fixture(scope="module")
def own_dist(data):
    """The restatement's distances of the train rows among themselves, shared by the leave-one-out and the self-audit tests"""
    train, _ = data
    return ref.distances(train.ids, train.lengths, train.ids, train.lengths, 192)


@pytest.fixture(scope="module")
def knn(data):
    import slnlp
    return slnlp.EditKNN(k=5, max_len=192).fit(data[0])


def test_estimator_matches_restatement(data, expected, knn):
    import slnlp
    train, test = data
    with pytest.raises(ValueError, match=r"rows have a length outside 0..64 .*rows longer than 64 frames are refused, not truncated"):
        slnlp.EditKNN().fit(train)                           # today's message
    d, i = knn.kneighbors(test)
    assert d.dtype == np.int32 and i.dtype == np.int64
    _same(d, expected["res"]["nbr"][:, :, 0], "distances")
    _same(i, expected["res"]["nbr"][:, :, 1].astype(np.int64), "indices")
    assert d.max() > 64                                      # beyond what one byte of the 64-frame search's bound holds
    proba = knn.predict_proba(test)
    want = torch.softmax(torch.from_numpy(expected["logp"]), dim=-1).numpy()
    assert np.allclose(proba, want, rtol=0, atol=1e-6) and np.allclose(proba.sum(1), 1.0, atol=1e-5)
    logp = knn._forward_logp(test, lambda z, y: z.cpu().numpy())
    assert np.isfinite(logp).all() and (np.abs(logp - expected["logp"]) <= np.spacing(np.abs(expected["logp"]))).all()
    assert knn.get_params()["max_len"] == 192


def test_chunked_queries_give_the_same_bytes(data, knn):
    import copy
    from slnlp.edit_knn import query_chunks
    _, test = data
    whole = knn._forward_logp(test, lambda z, y: z.cpu().numpy())
    small = copy.copy(knn)
    small._cap = 2 * 200 * 40                                # two bytes a pair: 40 queries per chunk, three chunks, the last of 20
    assert query_chunks(100, 200, small._cap // 2) == [(0, 40), (40, 80), (80, 100)]
    assert whole.tobytes() == small._forward_logp(test, lambda z, y: z.cpu().numpy()).tobytes()
    assert np.array_equal(knn.kneighbors(test)[1], small.kneighbors(test)[1])


def test_leave_one_out_and_attribute(data, knn, own_dist):
    train, test = data
    loo = knn.leave_one_out()
    d, i = loo.kneighbors(train)
    assert (i != np.arange(len(train))[:, None]).all() and (i >= 0).all()
    want = ref.knn_rows(own_dist, train.lengths, train.lengths, 150, 150, 5, 192, exclude=np.arange(200))
    _same(d, want["nbr"][:, :, 0], "leave-one-out distances")
    rel = loo.reliability(train)
    assert rel["rows"] == 200 and rel["nan_rows"] == 0 and np.isfinite([rel["ece"], rel["nll"], rel["accuracy"]]).all()
    four = test[np.arange(4)]
    att = knn.attribute(four, by="frame")                    # the occluded variants are DeviceRows: through the long path too
    assert att["rows"] == 4 and np.isfinite(att["top_drop"]).all() and att["usable"] == int(four.lengths.sum())


def test_split_audit(data, expected, own_dist):
    import slnlp
    from slnlp import metrics
    train, test = data
    got = slnlp.split_audit(train, test, radius=80, top=20, max_len=192)
    res = ref.knn_rows(expected["dist"], test.lengths, train.lengths, 150, 150, 1, 192, radius=80)
    want = metrics.split_audit_report(res["rows"], res["nbr"], test.y, train.y, 80, 20, head=res["head"], max_distance=192)
    for key in ("rows", "exact_duplicates", "near_duplicates", "conflicting", "conflicting_exact", "pairs", "flagged_queries", "flagged_references"):
        assert got[key] == want[key], key
    assert got["nearest_hist"].shape == (194,) and np.array_equal(got["nearest_hist"], want["nearest_hist"]) and got["flagged_queries"] == 0
    assert got["nearest_hist"][65:193].sum() > 0 and got["self"] is False
    own = slnlp.split_audit(train, train, radius=80, max_len=192)
    loo = ref.knn_rows(own_dist, train.lengths, train.lengths, 150, 150, 1, 192, radius=80, exclude=np.arange(200))
    assert own["self"] is True and own["near_duplicates"] == int((loo["rows"][:, 2] <= 80).sum()) and all(q != r for q, r, *_ in own["pairs"])
    assert own["nearest_hist"][0] == int((loo["rows"][:, 2] == 0).sum())      # no row found its own copy
    short = slnlp.split_audit(train, test)                   # without max_len: today's audit, the long rows flagged
    assert short["nearest_hist"].shape == (66,) and short["flagged_queries"] == int((test.lengths > 64).sum()) > 0


def test_cli_baseline_files(data, tmp_path):
    import csv
    import json
    from slnlp import cli
    from test_attribution_gpu import make_net
    train, test = data
    torch.manual_seed(9)
    net = make_net(train, max_epochs=1).fit(train)           # one tiny fused fit: a one-epoch GRU
    opts = cli.baseline_options({"k": 5, "radius": 80, "top": 7, "max_len": 192})
    knn, audit = cli.save_baseline(net, train, test, opts, {"replicates": 100}, ["accuracy", "neg_log_loss"], "cuda", str(tmp_path))
    base = json.load(open(tmp_path / "test_baseline.json"))
    assert np.isfinite(base["scores"]["test_accuracy"]) and np.isfinite(base["scores"]["test_neg_log_loss"])
    assert base["options"]["k"] == 5 and base["options"]["max_len"] == 192 and base["train_rows"] == 200 and base["neighbours"]["rows"] == 100
    split = json.load(open(tmp_path / "test_split_audit.json"))
    assert split["rows"] == 100 and split["near_duplicates"] == audit["near_duplicates"] and len(split["nearest_hist"]) == 194
    assert split["flagged_queries"] == 0 and split["rows_duplicated"] + split["rows_clean"] == 100
    lines = list(csv.reader(open(tmp_path / "test_split_audit_rows.csv")))
    assert lines[0][:4] == ["row", "label", "name", "nearest"] and len(lines) == 101
