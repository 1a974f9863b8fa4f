"""GPU: phonology-weighted edit-distance neighbours on the device -- ``slnlp_field_distances``, ``slnlp_field_knn_rows`` and
``slnlp_field_knn_logp`` through ``slnlp.ops`` against the numpy restatement (tests/field_knn_ref.py), against the unit-cost kernels
at F = 1, then ``PhonoKNN``, ``split_audit(field_codes=...)`` and the CLI key ``phono_baseline`` end to end.

The bounds.  Distances (uint16), neighbours, the per-query rows and the head are integers and EQUAL the restatement's.  The vote is
held to the bound tests/test_edit_knn_gpu.py states and justifies, and no other: it is formed in fp64 in the restatement's order of
operations, the device's exp and log may differ from numpy's by an fp64 ulp, which moves the float32 rounding of log(p) by at most
one unit -- every finite entry lies within ONE float32 ulp of the restatement, NaN rows match exactly, and the arg-max equals the
restatement's wherever its top-two gap exceeds that ulp.  At F = 1 the vote is bit-equal to ``edit_knn_logp``'s.

The inputs.  Rows come from ``edit_knn_ref.make_rows``: they lie S + 3 tokens apart, and the padding and the tokens past a row's
length are live tokens, so a read past L changes a distance.  Cases with at least 8 queries and 9 references carry a query and a
reference of lengths 65 and -1, an ``exclude`` list with -1 entries and a duplicated reference whose twin the first query skips."""
import functools

import numpy as np
import pytest
import torch

import field_knn_ref as ref

pytestmark = pytest.mark.gpu

#         nq   nr   S   k   F  gap
SHAPES = [(1, 1, 1, 1, 1, 1),             # the smallest case
          (3, 2, 5, 4, 3, 1),             # k > nr, gap < F
          (8, 9, 64, 5, 16, 16),          # distances above 255 and above 512, the last bin 1024
          (65, 257, 48, 5, 6, 6),         # more references than a block's threads, queries past a wave; the reference config's F
          (129, 300, 64, 64, 2, 2),       # codes over 2 values per field: almost every distance tied, k at its cap
          (33, 40, 17, 5, 6, 3)]          # tokens 2^33 t + 7 and negative ones: all outside the table, equal only to themselves
IDS = [f"{nq}x{nr}x{S}k{k}F{F}g{gap}" for nq, nr, S, k, F, gap in SHAPES]
VT = 40


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _lengths(rs, n, S):
    """random ones, then S, 0, S - 1 and 1 in the last places (as far as n goes): the rows a case rewrites are the first six"""
    edge = np.array([S, 0, S - 1, 1], dtype=np.int64)[:n]
    return np.concatenate([rs.randint(0, S + 1, size=n - len(edge)), edge]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(index):
    """One shape's inputs and the restatement's outputs, formed once and shared (nobody writes to them)"""
    nq, nr, S, k, F, gap = SHAPES[index]
    rs = np.random.RandomState(200 + index)
    if index == 4:
        codes = rs.randint(0, 2, size=(VT, F)).astype(np.int32)
    else:
        codes = rs.randint(0, 4, size=(VT, F)).astype(np.int32)
    codes[0], codes[1] = 0, 1                                # tokens 0 and 1 differ in every field
    if index == 5:
        alphabet = np.concatenate([(np.arange(1, 5, dtype=np.int64) << 33) + 7, -np.arange(1, 4, dtype=np.int64)])
    else:
        alphabet = np.arange(0, VT + 2, dtype=np.int64)      # VT and VT + 1: just outside the table
    token = lambda m: rs.choice(alphabet, size=m)
    Xq, Lq = ref.make_rows(rs, nq, S, alphabet, _lengths(rs, nq, S), token)
    Xr, Lr = ref.make_rows(rs, nr, S, alphabet, _lengths(rs, nr, S), token)
    exclude = None
    if nq >= 8 and nr >= 9:
        Lr[0] = S if S >= 63 else max(Lr[0], min(S, 3))
        Xr[0, :Lr[0]] = token(Lr[0])
        Xr[5], Lr[5] = Xr[0], Lr[0]                          # a duplicated reference, and a query that equals both
        Xq[0], Lq[0] = Xr[0], Lr[0]
        Lq[1], Lq[3], Lr[2], Lr[4] = 65, -1, 65, -1
        if index == 2:                                       # 64 frames of token 0 against 64 of token 1, and against an empty row
            Xq[2, :S], Lq[2] = 0, S
            Xr[1, :S], Lr[1] = 1, S
            Lr[3] = 0
        exclude = np.where(rs.rand(nq) < 0.5, -1, rs.randint(0, nr, size=nq)).astype(np.int64)
        exclude[0], exclude[2] = 0, -1                       # query 0 skips its twin 0 and finds the copy 5
    dist = ref.distances(Xq, Lq, Xr, Lr, codes, gap)
    radius = F
    res = ref.knn_rows(dist, Lq, Lr, S + 3, S + 3, k, F, radius=radius, exclude=exclude)
    return dict(nq=nq, nr=nr, S=S, k=k, F=F, gap=gap, codes=codes, radius=radius, Xq=Xq, Lq=Lq, Xr=Xr, Lr=Lr, exclude=exclude, dist=dist, res=res)


def _device_rows(c):
    """The rows as the device sees them: [n, S] views of tensors whose rows lie S + 3 apart"""
    S = c["S"]
    return _dev(c["Xq"])[:, :S], _dev(c["Lq"]), _dev(c["Xr"])[:, :S], _dev(c["Lr"])


def _search(c, sl=slice(None)):
    from slnlp import ops
    Xq, Lq, Xr, Lr = _device_rows(c)
    ex = None if c["exclude"] is None else _dev(c["exclude"])[sl]
    return ops.field_knn_rows(Xq[sl], Lq[sl], Xr, Lr, _dev(c["codes"]), c["k"], gap=c["gap"], radius=c["radius"], exclude=ex)


# ---------------------------------------------------------------------------------------------------------- integers ----
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=IDS)
def test_distances_equal_restatement(index):
    from slnlp import ops
    c = case(index)
    got = ops.field_distances(*_device_rows(c), _dev(c["codes"]), c["gap"]).cpu().numpy()
    assert got.dtype == np.uint16 and got.shape == (c["nq"], c["nr"])
    wrong = np.argwhere(got != c["dist"])
    assert wrong.size == 0, f"{len(wrong)} of {got.size} distances differ, first at {wrong[0]}: {got[tuple(wrong[0])]} != {c['dist'][tuple(wrong[0])]}"


@pytest.mark.parametrize("index", range(len(SHAPES)), ids=IDS)
def test_neighbours_equal_restatement(index):
    from slnlp import ops
    c = case(index)
    got = ops.edit_knn_download(_search(c))
    want = c["res"]
    assert np.array_equal(got["rows"], want["rows"])
    assert np.array_equal(got["nbr"], want["nbr"])
    assert np.array_equal(got["head"], want["head"])
    if c["exclude"] is not None:                             # what the case was built to hold
        assert got["head"][0] == 2 and got["head"][1] == 2 and (want["rows"][[1, 3], 3] == 1).all() and (want["nbr"][[1, 3]] == -1).all()
        assert tuple(want["nbr"][0, 0]) == (0, 5)
    if c["k"] > c["nr"]:
        assert (want["rows"][:, 0] < c["k"]).all() and (want["nbr"][:, c["nr"]:] == -1).all()


@pytest.mark.parametrize("F", [4, 5, 8, 9, 12, 13])
def test_every_group_count_of_the_kernel(F):
    """The distance kernel is built once per number of groups of four fields: F on both sides of every threshold (1 and 16 above)"""
    from slnlp import ops
    rs = np.random.RandomState(300 + F)
    codes = rs.randint(0, 3, size=(VT, F)).astype(np.int32)
    alphabet = np.arange(0, VT + 2, dtype=np.int64)
    token = lambda m: rs.choice(alphabet, size=m)
    Xq, Lq = ref.make_rows(rs, 9, 11, alphabet, _lengths(rs, 9, 11), token)
    Xr, Lr = ref.make_rows(rs, 20, 11, alphabet, _lengths(rs, 20, 11), token)
    gap = 1 + F // 2
    want = ref.distances(Xq, Lq, Xr, Lr, codes, gap)
    got = ops.field_distances(_dev(Xq)[:, :11], _dev(Lq), _dev(Xr)[:, :11], _dev(Lr), _dev(codes), gap).cpu().numpy()
    assert np.array_equal(got, want) and want.max() > F


def test_what_the_sixteen_field_case_holds():
    c = case(2)
    d = c["dist"]
    assert d[2, 1] == 1024 and d[2, 3] == 1024               # every field of 64 frames differs; 64 frames against none
    fin = d[d != 65535]
    assert (fin > 255).any() and (fin > 512).any() and fin.max() == 1024
    assert sorted(set(c["Lq"]) | set(c["Lr"])) [:2] == [-1, 0] and {1, 63, 64, 65} <= set(c["Lq"]) | set(c["Lr"])
    assert (d[1] == 65535).all() and (d[:, 2] == 65535).all()
    assert (c["res"]["nbr"][2, :, 0] >= 0).all() and c["res"]["rows"][2, 2] <= 1024


def test_ties_dominate_the_two_value_case():
    c = case(4)
    kth = c["res"]["nbr"][:, c["k"] - 1, 0]
    tied = [(c["dist"][i] == kth[i]).sum() > 1 for i in range(c["nq"]) if kth[i] >= 0]
    assert np.mean(tied) > 0.9


def test_tokens_outside_the_table_equal_only_themselves():
    c = case(5)
    assert ((c["Xq"] < 0) | (c["Xq"] >= VT)).all() and ((c["Xr"] < 0) | (c["Xr"] >= VT)).all()
    i, j = 6, 7                                              # by hand: every substitution costs F = 6 or 0, a gap 3
    assert c["dist"][i, j] == ref.distance(c["codes"], c["gap"], c["Xq"][i, :c["Lq"][i]], c["Xr"][j, :c["Lr"][j]])


# ------------------------------------------------------------------------------------------ two kernels, one answer ----
def test_one_field_equals_the_unit_cost_kernels():
    """F = 1, codes[v] = v, gap = 1 on the rows of the unit-cost suite's 65 x 257 case: the same distances (255 <-> 65535), the
    same neighbours, bit-equal votes"""
    import test_edit_knn_gpu as unit
    from slnlp import ops
    c = unit.case(4)
    Xq, Lq, Xr, Lr = unit._device_rows(c)
    codes = _dev(np.arange(64, dtype=np.int32)[:, None])     # the alphabet is 2..39
    d1 = ops.edit_distances(Xq, Lq, Xr, Lr).cpu().numpy().astype(np.int64)
    dF = ops.field_distances(Xq, Lq, Xr, Lr, codes, 1).cpu().numpy().astype(np.int64)
    assert np.array_equal(np.where(d1 == 255, 65535, d1), dF) and (d1 == 255).any()
    ex = _dev(c["exclude"])
    b1 = ops.edit_knn_rows(Xq, Lq, Xr, Lr, c["k"], radius=unit.RADIUS, exclude=ex)
    bF = ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, c["k"], gap=1, radius=unit.RADIUS, exclude=ex)
    g1, gF = ops.edit_knn_download(b1), ops.edit_knn_download(bF)
    for name in ("head", "rows", "nbr"):
        assert g1[name].tobytes() == gF[name].tobytes(), name
    yr = _dev(np.random.RandomState(3).randint(0, 9, size=c["nr"]).astype(np.int64))
    prior = _dev(np.full(9, 1.0 / 9))
    for weights in ("uniform", "distance"):
        for normalize in (False, True):
            z1 = ops.edit_knn_logp(b1, Lq, Lr, yr, prior, weights=weights, tau=0.75, normalize=normalize, lam=0.5).cpu().numpy()
            zF = ops.field_knn_logp(bF, Lq, Lr, yr, prior, 1, weights=weights, tau=0.75, normalize=normalize, lam=0.5).cpu().numpy()
            assert z1.tobytes() == zF.tobytes(), (weights, normalize)


# ------------------------------------------------------------------------------------------------------------- votes ----
@pytest.mark.parametrize("weights", ["uniform", "distance"])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("index,V", [(2, 7), (3, 70), (4, 7)], ids=["8x9", "65x257", "129x300"])
def test_votes_within_one_float32_ulp(index, V, normalize, weights):
    from slnlp import ops
    c = case(index)
    rs = np.random.RandomState(7 + index)
    yr = rs.randint(0, V, size=c["nr"]).astype(np.int64)
    yr[1], yr[3], yr[5] = -1, V, -1                          # labels outside the classes: skipped and counted (5: query 0's nearest)
    prior = ref.prior_of(yr[(yr >= 0) & (yr < V)], V)
    tau, lam = 0.75, 0.5
    want, bad = ref.knn_logp(c["res"], c["Lq"], c["Lr"], yr, prior, c["F"], weights=weights, tau=tau, normalize=normalize, lam=lam)
    buf = _search(c)
    out = torch.full((c["nq"], V + 3), 7.0, dtype=torch.float32, device="cuda")          # padded rows: the padding stays
    ops.field_knn_logp(buf, _dev(c["Lq"]), _dev(c["Lr"]), _dev(yr), _dev(prior), c["F"], weights=weights, tau=tau, normalize=normalize, lam=lam,
                       out=out[:, :V])
    full = out.cpu().numpy()
    got = full[:, :V]
    assert (full[:, V:] == 7.0).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want).all(axis=1).sum() == c["res"]["head"][0] == 2
    fin = ~np.isnan(want)
    assert np.isfinite(want[fin]).all() and np.isfinite(got[fin]).all()
    ulp = np.spacing(np.abs(want[fin]))
    print(f"\n{(got[fin] != want[fin]).sum()} of {fin.sum()} entries differ from the restatement; largest {np.max(np.abs(got[fin] - want[fin]) / ulp):.2f} ulp")
    assert (np.abs(got[fin] - want[fin]) <= ulp).all()
    rows = fin.all(axis=1)
    top2 = np.sort(want[rows], axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > np.spacing(np.abs(top2[:, 1]))
    assert np.array_equal(got[rows].argmax(1)[clear], want[rows].argmax(1)[clear])
    assert int(ops.edit_knn_download(buf, neighbours=False)["head"][2]) == bad and bad > 0


# ------------------------------------------------------------------------------------------------------ equal bytes ----
def test_equal_bytes_across_runs_and_beside_the_unit_cost_search():
    """Two runs of the 65 x 257 case, one alone and one while a second stream runs the unit-cost search on the same rows"""
    from slnlp import ops
    c = case(3)
    Xq, Lq, Xr, Lr = _device_rows(c)
    codes, ex = _dev(c["codes"]), _dev(c["exclude"])
    yr = _dev(np.random.RandomState(3).randint(0, 9, size=c["nr"]).astype(np.int64))
    prior = _dev(np.full(9, 1.0 / 9))

    def run():
        scratch = torch.empty(2 * c["nq"] * c["nr"], dtype=torch.uint8, device="cuda")
        buf = ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, c["k"], gap=c["gap"], radius=c["radius"], exclude=ex, scratch=scratch)
        z = ops.field_knn_logp(buf, Lq, Lr, yr, prior, c["F"])
        return buf, z, scratch
    torch.cuda.synchronize()
    a = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # queued first: it runs while the second field search is enqueued
        for _ in range(4):
            other = ops.edit_knn_rows(Xq, Lq, Xr, Lr, c["k"], radius=2, exclude=ex)
    b = run()
    side.synchronize()
    torch.cuda.synchronize()
    ga, gb = ops.edit_knn_download(a[0]), ops.edit_knn_download(b[0])
    for name in ("head", "rows", "nbr"):
        assert ga[name].tobytes() == gb[name].tobytes(), name
    assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
    assert a[2].cpu().numpy().tobytes() == b[2].cpu().numpy().tobytes()                  # the uint16 matrix itself
    assert np.array_equal(ga["nbr"], c["res"]["nbr"]) and ops.edit_knn_download(other)["rows"].shape == (c["nq"], 4)


# -------------------------------------------------------------------------------------------------------- refusals ----
def test_library_refusals():
    """Each refusal comes from the library -- the ctypes table is called directly, past the checks of ``slnlp.ops`` -- returns an
    error code and names its entry point"""
    from slnlp import _lib, ops
    lib = _lib.load()
    c = case(1)
    Xq, Lq, Xr, Lr = _device_rows(c)
    codes = _dev(c["codes"])
    buf = ops.edit_knn_buffers(c["nq"], 2, Xq.device)
    scratch = torch.empty(2 * c["nq"] * c["nr"] + 8, dtype=torch.uint8, device="cuda")
    dist = torch.empty(c["nq"], c["nr"], dtype=torch.uint16, device="cuda")
    p, st = ops.ptr, ops.stream_ptr()

    def rows(F=3, gap=1, radius=0, table=None, scratch_bytes=None, codes_ptr=None):
        return lib.slnlp_field_knn_rows(p(Xq), int(Xq.stride(0)), p(Lq), c["nq"], p(Xr), int(Xr.stride(0)), p(Lr), c["nr"],
                                        p(codes) if codes_ptr is None else codes_ptr, VT, F, gap, None, 2, radius, p(scratch),
                                        scratch.numel() if scratch_bytes is None else scratch_bytes, p(buf["head"]), p(buf["rows"]), p(buf["nbr"]), st)

    def distances(F=3, gap=1, codes_ptr=None, dist_ptr=None):
        return lib.slnlp_field_distances(p(Xq), int(Xq.stride(0)), p(Lq), c["nq"], p(Xr), int(Xr.stride(0)), p(Lr), c["nr"],
                                         p(codes) if codes_ptr is None else codes_ptr, VT, F, gap, p(dist) if dist_ptr is None else dist_ptr, st)

    def refused(rc, text):
        msg = lib.slnlp_last_error().decode()
        assert rc != 0 and text in msg, (rc, msg)
    one = p(codes) + 1
    refused(rows(F=0), "field_knn_rows: F=0 outside 1..16")
    refused(rows(F=17), "field_knn_rows: F=17 outside 1..16")
    refused(rows(gap=0), "field_knn_rows: gap=0 outside 1..F=3")
    refused(rows(gap=4), "field_knn_rows: gap=4 outside 1..F=3")
    refused(rows(radius=64 * 3 + 1), "field_knn_rows: radius=193 outside 0..64 F=192")
    refused(rows(codes_ptr=one), "field_knn_rows: misaligned pointer (codes: 4 bytes)")
    refused(rows(scratch_bytes=3), "field_knn_rows: scratch of 3 bytes is too small")
    refused(rows(codes_ptr=p(scratch)), "field_knn_rows: output scratch overlaps input codes")
    refused(distances(F=0), "field_distances: F=0 outside 1..16")
    refused(distances(F=17), "field_distances: F=17 outside 1..16")
    refused(distances(gap=0), "field_distances: gap=0 outside 1..F=3")
    refused(distances(gap=4), "field_distances: gap=4 outside 1..F=3")
    refused(distances(codes_ptr=one), "field_distances: misaligned pointer (codes: 4 bytes)")
    refused(distances(dist_ptr=p(dist) + 1), "field_distances: misaligned pointer (dist: 2 bytes)")
    prior = _dev(np.full(3, 1 / 3))
    rc = lib.slnlp_field_knn_logp(p(buf["nbr"]), p(buf["rows"]), p(Lq), p(Lr), p(Lr), c["nq"], c["nr"], 2, 3, 17, 1, 1.0, 1, 1.0, p(prior),
                                  p(torch.empty(c["nq"], 3, device="cuda")), 3, p(buf["head"]), st)
    refused(rc, "field_knn_logp: F=17 outside 1..16")
    assert lib.slnlp_field_knn_scratch_bytes(3, 5) == 30 and lib.slnlp_field_knn_scratch_bytes(0, 5) == -1
    assert "field_knn_scratch_bytes" in lib.slnlp_last_error().decode()
    with pytest.raises(RuntimeError, match="field_knn_rows: scratch of 3 bytes is too small"):
        ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, 2, scratch=torch.empty(3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="field_knn_rows: radius=193"):
        ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, 2, radius=193)
    assert rows() == 0                                       # and the same call with nothing wrong goes through
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ end to end ----
@pytest.fixture(scope="module")
def data():
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(400, seq_len=12, src_vocab=64, n_labels=6, seed=5, min_len=3)
    return ds[np.arange(300)], ds[np.arange(300, 400)]


@pytest.fixture(scope="module")
def table():
    """A made-up [64, 3] table: token v has the parts (v mod 4, (v / 4) mod 4, v / 16) -- v and v ^ 1 differ in one field"""
    v = np.arange(64)
    return np.stack([v % 4, (v // 4) % 4, v // 16], axis=1).astype(np.int32)


@pytest.fixture(scope="module")
def expected(data, table):
    """The restatement on the end-to-end data: distances, the 5 neighbours, PhonoKNN's default vote"""
    train, test = data
    V, S = len(train.vocab_y), train.ids.shape[1]
    dist = ref.distances(test.ids, test.lengths, train.ids, train.lengths, table, 3)
    res = ref.knn_rows(dist, test.lengths, train.lengths, S, S, 5, 3)
    logp, _ = ref.knn_logp(res, test.lengths, train.lengths, train.y, ref.prior_of(train.y, V), 3)
    return dict(dist=dist, res=res, logp=logp)


@pytest.fixture(scope="module")
def knn(data, table):
    import slnlp
    return slnlp.PhonoKNN(table, k=5).fit(data[0])


def test_estimator_matches_restatement(data, table, expected, knn):
    import copy
    train, test = data
    assert knn.fields_ == 3 and np.array_equal(knn.classes_, np.arange(len(train.vocab_y)))
    d, i = knn.kneighbors(test)
    assert d.dtype == np.int32 and i.dtype == np.int64
    assert np.array_equal(d, expected["res"]["nbr"][:, :, 0]) and np.array_equal(i, expected["res"]["nbr"][:, :, 1])
    proba = knn.predict_proba(test)
    want = torch.softmax(torch.from_numpy(expected["logp"]), dim=-1).numpy()
    assert np.allclose(proba, want, rtol=0, atol=1e-6) and np.allclose(proba.sum(1), 1.0, atol=1e-5)
    assert np.array_equal(knn.predict(test), expected["logp"].argmax(1))
    small = copy.copy(knn)
    small._cap = 300 * 14                                    # two bytes a pair: 7 queries per chunk, 15 chunks, the last of 2
    whole = knn._forward_logp(test, lambda z, y: z.cpu().numpy())
    assert whole.tobytes() == small._forward_logp(test, lambda z, y: z.cpu().numpy()).tobytes()
    assert np.array_equal(small.kneighbors(test)[1], i)


def test_leave_one_out_and_the_diagnostics_run_on_it(data, table, knn):
    train, test = data
    S = train.ids.shape[1]
    loo = knn.leave_one_out()
    d, i = loo.kneighbors(train)
    own = ref.distances(train.ids, train.lengths, train.ids, train.lengths, table, 3)
    want = ref.knn_rows(own, train.lengths, train.lengths, S, S, 5, 3, exclude=np.arange(300))
    assert np.array_equal(d, want["nbr"][:, :, 0]) and np.array_equal(i, want["nbr"][:, :, 1]) and (i != np.arange(300)[:, None]).all()
    rel = knn.reliability(test)
    assert rel["rows"] == 100 and np.isfinite([rel["ece"], rel["nll"], rel["accuracy"]]).all() and rel["nan_rows"] == 0
    assert len(loo.label_issues(train)["issues"]["row"]) <= 300


def test_compare_with_the_unit_cost_baseline(data, knn):
    import slnlp
    train, test = data
    unit = slnlp.EditKNN(k=5).fit(train)
    a = unit.compare(knn, test, scoring=["accuracy", "neg_log_loss"], replicates=200, seed=11)
    b = knn.compare(unit, test, scoring=["accuracy", "neg_log_loss"], replicates=200, seed=11)
    for name in ("accuracy", "neg_log_loss"):
        assert a[name]["point"] == pytest.approx(-b[name]["point"]) and a[name]["lower"] == pytest.approx(-b[name]["upper"])
    assert a["neg_log_loss"]["point"] != 0.0


def test_split_audit_in_field_units(data, table, expected, knn):
    import slnlp
    from slnlp import metrics
    from slnlp.data import TokenDataset
    train, test = data
    S = train.ids.shape[1]
    got = slnlp.split_audit(train, test, radius=5, top=20, judge=knn, field_codes=table)
    res = ref.knn_rows(expected["dist"], test.lengths, train.lengths, S, S, 1, 3, radius=5)
    want = metrics.split_audit_report(res["rows"], res["nbr"], test.y, train.y, 5, 20, head=res["head"], max_distance=192)
    for key in ("rows", "exact_duplicates", "near_duplicates", "conflicting", "conflicting_exact", "pairs", "flagged_queries", "flagged_references"):
        assert got[key] == want[key], key
    assert got["nearest_hist"].shape == (194,) and np.array_equal(got["nearest_hist"], want["nearest_hist"])
    assert np.array_equal(got["duplicated"], want["duplicated"]) and got["self"] is False
    assert got["rows_duplicated"] + got["rows_clean"] == 100
    # one field of one frame: distance 1 here, a whole edit for the unit-cost audit
    ids = train.ids[7:8].copy()
    assert train.lengths[7] >= 2
    ids[0, 1] ^= 1
    probe = TokenDataset(ids, train.lengths[7:8], train.y[7:8], train.vocab_X, train.vocab_y)
    near = slnlp.split_audit(train, probe, radius=1, field_codes=table)
    assert near["near_duplicates"] == 1 and near["exact_duplicates"] == 0 and near["pairs"][0][:3] == (0, 7, 1)
    unit = slnlp.split_audit(train, probe, radius=0)
    assert unit["near_duplicates"] == 0 and not unit["duplicated"][0]


def test_cli_phono_baseline_files(data, table, tmp_path):
    import csv
    import json
    import slnlp
    from slnlp import cli
    from test_attribution_gpu import make_net
    train, test = data
    torch.manual_seed(9)
    net = make_net(train, max_epochs=1).fit(train)
    unit = slnlp.EditKNN(k=5).fit(train)
    opts = cli.phono_baseline_options({"k": 5, "top": 7})
    knn, audit = cli.save_phono_baseline(net, train, test, opts, None, {"replicates": 100}, ["accuracy", "neg_log_loss"], "cuda", str(tmp_path),
                                         unit=unit, field_codes=table)
    base = json.load(open(tmp_path / "test_phono_baseline.json"))
    assert np.isfinite([base["scores"]["test_accuracy"], base["scores"]["test_neg_log_loss"]]).all()
    assert base["options"] == {"k": 5, "weights": "distance", "tau": 1.0, "normalize": True, "smoothing": 1.0, "gap": 3, "fields": 3}
    assert base["train_rows"] == 300 and base["neighbours"]["rows"] == 100 and len(base["neighbours"]["nearest_hist"]) == 194
    assert set(base["refit_vs_phono"]) >= {"accuracy", "neg_log_loss", "replicates"} and set(base["baseline_vs_phono"]) >= {"accuracy", "neg_log_loss"}
    split = json.load(open(tmp_path / "test_phono_split_audit.json"))
    assert split["rows"] == 100 and split["radius"] == 3 and split["near_duplicates"] == audit["near_duplicates"] and len(split["nearest_hist"]) == 194
    assert split["rows_duplicated"] + split["rows_clean"] == 100 and len(split["pairs"]) <= 7 and split["gap"] == 3 and split["fields"] == 3
    lines = list(csv.reader(open(tmp_path / "test_phono_split_audit_rows.csv")))
    assert lines[0][:4] == ["row", "label", "name", "nearest"] and len(lines) == 101
    assert sum(int(r[7]) for r in lines[1:]) == split["near_duplicates"]
