"""GPU: per-field integer weights of the phonology-weighted edit distance -- ``slnlp_field_distances_w`` / ``slnlp_field_knn_rows_w``
and ``slnlp_loo_objective`` through ``slnlp.ops`` against the numpy restatement (tests/field_weight_ref.py), against the unweighted
kernels at all ones, then ``PhonoKNN(field_weights=)``, ``split_audit(field_weights=)``, ``fit_field_weights`` and the CLI sub-key
end to end.

The bounds.  Distances, neighbours, the per-query rows, the head and the objective's counts are integers and EQUAL the
restatement's.  The vote is held to the bound tests/test_edit_knn_gpu.py states and justifies -- every finite entry within ONE
float32 ulp of the restatement.  The objective's fp64 sum over given log-probs is a fixed tree and equals the restatement's bit
for bit; over the device's own log-probs it lies within N 2^-23 max|logp| of the restatement's (one float32 ulp per picked entry).

The inputs.  Rows come from ``edit_knn_ref.make_rows`` (the cases of tests/test_field_knn_gpu.py are reused as they are): they lie
S + 3 tokens apart and the tokens past a row's length are live."""
import functools

import numpy as np
import pytest
import torch

import field_knn_ref as unit_ref
import field_weight_ref as ref

pytestmark = pytest.mark.gpu

VT = 40


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _rows(c):
    S = c["S"]
    return _dev(c["Xq"])[:, :S], _dev(c["Lq"]), _dev(c["Xr"])[:, :S], _dev(c["Lr"])


def _unit_case(index):
    import test_field_knn_gpu as unit
    return unit.case(index)


#        name            rows of the unweighted suite's case, weights, gap, k
CASES = {"1x1x1": (0, (1,), 1, 1),
         "3x2x5 k>nr gap<W": (1, (2, 0, 1), 1, 4),
         "8x9x64 ones": (2, (1,) * 16, 16, 5),
         "8x9x64 last lane": (2, (0,) * 15 + (16,), 16, 5),
         "65x257x48 gap W": (3, (4, 0, 2, 0, 1, 3), 10, 5),
         "65x257x48 gap 1": (3, (4, 0, 2, 0, 1, 3), 1, 5),
         "33x40x17 outside W=3": (5, (1, 0, 2, 0, 0, 0), 3, 5),
         "33x40x17 outside W=12": (5, (4, 0, 2, 0, 3, 3), 12, 5)}


@functools.lru_cache(maxsize=None)
def case(name):
    """A weighted case on the rows of the unweighted suite: the restatement's distances and selection, formed once and shared"""
    index, w, gap, k = CASES[name]
    c = dict(_unit_case(index))
    W = sum(w)
    dist = ref.distances(c["Xq"], c["Lq"], c["Xr"], c["Lr"], c["codes"], w, gap)
    res = ref.knn_rows(dist, c["Lq"], c["Lr"], c["S"] + 3, c["S"] + 3, k, W, radius=W, exclude=c["exclude"])
    c.update(w=w, W=W, gap=gap, k=k, radius=W, dist=dist, res=res)
    return c


def _search(c, **more):
    from slnlp import ops
    Xq, Lq, Xr, Lr = _rows(c)
    ex = None if c["exclude"] is None else _dev(c["exclude"])
    return ops.field_knn_rows(Xq, Lq, Xr, Lr, _dev(c["codes"]), c["k"], gap=c["gap"], radius=c["radius"], exclude=ex, field_weights=c["w"], **more)


# ---------------------------------------------------------------------------------------------------------- integers ----
@pytest.mark.parametrize("name", list(CASES))
def test_distances_and_neighbours_equal_restatement(name):
    from slnlp import ops
    c = case(name)
    got = ops.field_distances(*_rows(c), _dev(c["codes"]), c["gap"], field_weights=c["w"]).cpu().numpy()
    assert got.dtype == np.uint16 and got.shape == c["dist"].shape
    wrong = np.argwhere(got != c["dist"])
    assert wrong.size == 0, f"{len(wrong)} of {got.size} distances differ, first at {wrong[0]}: {got[tuple(wrong[0])]} != {c['dist'][tuple(wrong[0])]}"
    out = ops.edit_knn_download(_search(c))
    for key in ("rows", "nbr", "head"):
        assert np.array_equal(out[key], c["res"][key]), key
    fin = c["dist"][c["dist"] != 65535]
    assert fin.max() <= 64 * c["W"]
    if c["k"] > c["Xr"].shape[0]:
        assert (c["res"]["rows"][:, 0] < c["k"]).all()
    if c["exclude"] is not None:                             # flagged rows, the exclude list and the duplicated reference
        assert out["head"][0] == 2 and out["head"][1] == 2 and tuple(c["res"]["nbr"][0, 0]) == (0, 5)


def test_what_the_sixteen_field_cases_hold():
    """64 frames of token 0 against 64 of token 1 (they differ in every field): 1024 with all ones -- the last bin -- and with 16 on
    field 15 alone, the last lane of the last group; 0 when the weight sits on a field in which the two agree"""
    from slnlp import ops
    ones, last = case("8x9x64 ones"), case("8x9x64 last lane")
    assert ones["dist"][2, 1] == 1024 and last["dist"][2, 1] == 1024 and ones["W"] == last["W"] == 16
    codes = last["codes"].copy()
    codes[1, 7] = codes[0, 7]
    w = (0,) * 7 + (16,) + (0,) * 8
    want = ref.distances(last["Xq"], last["Lq"], last["Xr"], last["Lr"], codes, w, 16)
    got = ops.field_distances(*_rows(last), _dev(codes), 16, field_weights=w).cpu().numpy()
    assert np.array_equal(got, want) and got[2, 1] == 0 and got[2, 3] == 1024          # against the empty row: 64 gaps of 16


@pytest.mark.parametrize("F", [4, 5, 8, 9, 12, 13])
def test_the_last_field_of_every_group_count(F):
    """The only non-zero weight on the LAST field: a group cut off too early gives all-zero distances between distinct tokens"""
    from slnlp import ops
    rs = np.random.RandomState(400 + F)
    codes = rs.randint(0, 3, size=(VT, F)).astype(np.int32)
    alphabet = np.arange(0, VT, dtype=np.int64)              # in-table tokens only
    token = lambda m: rs.choice(alphabet, size=m)
    Xq, Lq = ref.make_rows(rs, 9, 11, alphabet, np.full(9, 11), token)
    Xr, Lr = ref.make_rows(rs, 20, 11, alphabet, np.full(20, 11), token)
    w = (0,) * (F - 1) + (3,)
    want = ref.distances(Xq, Lq, Xr, Lr, codes, w, 3)
    got = ops.field_distances(_dev(Xq)[:, :11], _dev(Lq), _dev(Xr)[:, :11], _dev(Lr), _dev(codes), 3, field_weights=w).cpu().numpy()
    assert np.array_equal(got, want) and want.max() > 0


@pytest.mark.parametrize("name", ["33x40x17 outside W=3", "33x40x17 outside W=12"])
def test_a_token_outside_the_table_costs_W_never_F(name):
    c = case(name)
    assert ((c["Xq"] < 0) | (c["Xq"] >= VT)).all() and c["codes"].shape[1] == 6 and c["W"] != 6
    fin = c["dist"][c["dist"] != 65535]
    assert (fin % c["W"] == 0).all() and fin.max() > 0       # every substitution and every gap costs W here
    i, j = 6, 7
    assert c["dist"][i, j] == ref.distance(c["codes"], c["w"], c["gap"], c["Xq"][i, :c["Lq"][i]], c["Xr"][j, :c["Lr"][j]])


# ------------------------------------------------------------------------------------------ two kernels, one answer ----
@pytest.mark.parametrize("index", range(6))
def test_all_ones_equals_the_unweighted_kernels(index):
    """On each shape of tests/test_field_knn_gpu.py the weighted kernels with ones give the bytes of the unweighted ones"""
    from slnlp import ops
    c = _unit_case(index)
    Xq, Lq, Xr, Lr = _rows(c)
    codes = _dev(c["codes"])
    ones = (1,) * c["F"]
    d0 = ops.field_distances(Xq, Lq, Xr, Lr, codes, c["gap"]).cpu().numpy()
    d1 = ops.field_distances(Xq, Lq, Xr, Lr, codes, c["gap"], field_weights=ones).cpu().numpy()
    assert d0.tobytes() == d1.tobytes() and np.array_equal(d0, c["dist"])
    ex = None if c["exclude"] is None else _dev(c["exclude"])
    b0 = ops.edit_knn_download(ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, c["k"], gap=c["gap"], radius=c["radius"], exclude=ex))
    b1 = ops.edit_knn_download(ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, c["k"], gap=c["gap"], radius=c["radius"], exclude=ex, field_weights=ones))
    for key in ("head", "rows", "nbr"):
        assert b0[key].tobytes() == b1[key].tobytes(), key


def test_doubled_weights_double_the_distances_and_keep_the_votes():
    import slnlp
    from slnlp import ops
    c = case("65x257x48 gap W")
    Xq, Lq, Xr, Lr = _rows(c)
    codes, ex = _dev(c["codes"]), _dev(c["exclude"])
    w1 = (2, 0, 1, 0, 1, 3)                                  # W = 7, 2 W = 14
    w2 = tuple(2 * v for v in w1)
    a = ops.edit_knn_download(ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, 5, exclude=ex, field_weights=w1))
    b = ops.edit_knn_download(ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, 5, exclude=ex, field_weights=w2))
    assert np.array_equal(a["nbr"][:, :, 1], b["nbr"][:, :, 1]) and np.array_equal(np.where(a["nbr"][:, :, 0] < 0, -1, 2 * a["nbr"][:, :, 0]), b["nbr"][:, :, 0])
    assert (a["nbr"][:, :, 0] > 0).any()
    train, test = _end_to_end_data()
    table = _end_to_end_table()
    za = slnlp.PhonoKNN(table, field_weights=(2, 0, 1)).fit(train)._forward_logp(test, lambda z, y: z.cpu().numpy())
    zb = slnlp.PhonoKNN(table, field_weights=(4, 0, 2)).fit(train)._forward_logp(test, lambda z, y: z.cpu().numpy())
    assert za.tobytes() == zb.tobytes() and np.isfinite(za).all()        # 2 is a power of two: every fp64 quotient is the same


# ------------------------------------------------------------------------------------------------------------- votes ----
@pytest.mark.parametrize("normalize", [False, True])
def test_votes_within_one_float32_ulp(normalize):
    from slnlp import ops
    c = case("65x257x48 gap 1")
    V = 70
    rs = np.random.RandomState(17)
    yr = rs.randint(0, V, size=c["Xr"].shape[0]).astype(np.int64)
    prior = ref.prior_of(yr, V)
    want, _ = ref.knn_logp(c["res"], c["Lq"], c["Lr"], yr, prior, c["W"], tau=0.75, normalize=normalize, lam=0.5)
    got = ops.field_knn_logp(_search(c), _dev(c["Lq"]), _dev(c["Lr"]), _dev(yr), _dev(prior), c["W"], tau=0.75, normalize=normalize, lam=0.5).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).all(axis=1).sum() == 2
    fin = ~np.isnan(want)
    ulp = np.spacing(np.abs(want[fin]))
    print(f"\n{(got[fin] != want[fin]).sum()} of {fin.sum()} entries differ; largest {np.max(np.abs(got[fin] - want[fin]) / ulp):.2f} ulp")
    assert (np.abs(got[fin] - want[fin]) <= ulp).all()


# ------------------------------------------------------------------------------------------------------ equal bytes ----
def test_equal_bytes_across_runs_and_beside_the_unweighted_search():
    from slnlp import ops
    c = case("65x257x48 gap W")
    Xq, Lq, Xr, Lr = _rows(c)
    codes, ex = _dev(c["codes"]), _dev(c["exclude"])
    nq, nr = c["dist"].shape

    def run():
        scratch = torch.empty(2 * nq * nr, dtype=torch.uint8, device="cuda")
        buf = ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, c["k"], gap=c["gap"], radius=c["radius"], exclude=ex, scratch=scratch, field_weights=c["w"])
        return buf, scratch
    torch.cuda.synchronize()
    a = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # queued first: it runs while the weighted search is enqueued
        for _ in range(4):
            other = ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, c["k"], exclude=ex)
    b = run()
    side.synchronize()
    torch.cuda.synchronize()
    ga, gb = ops.edit_knn_download(a[0]), ops.edit_knn_download(b[0])
    for key in ("head", "rows", "nbr"):
        assert ga[key].tobytes() == gb[key].tobytes(), key
    assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()                  # the uint16 matrix itself
    assert np.array_equal(ga["nbr"], c["res"]["nbr"])
    assert np.array_equal(ops.edit_knn_download(other)["nbr"], _unit_case(3)["res"]["nbr"])


# ---------------------------------------------------------------------------------------------------- the objective ----
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_loo_objective_against_numpy(N):
    from slnlp import ops
    V = 7
    rs = np.random.RandomState(N)
    z = np.log(rs.dirichlet(np.ones(V), size=N)).astype(np.float32)
    y = rs.randint(0, V, size=N).astype(np.int64)
    if N >= 63:
        z[3, 2] = z[3, 5] = z[3].max() + 1.0                 # a tie at the top: column 2 wins
        y[3] = 5                                             # ... so the label 5 is wrong
        z[4, 1] = z[4, 6] = z[4].max() + 1.0
        y[4] = 1                                             # ... and the label 1 is right
        z[7] = np.nan                                        # a flagged query's row
        z[9, 0] = np.nan
        y[11], y[12] = -1, V                                 # labels outside the classes
        z[13, y[13]] = z[13].min() - 50.0                    # a large term
    want = ref.loo_objective(z, y)
    table = ops.loo_objective_table(3, "cuda")
    pad = torch.full((N, V + 2), 9.0, dtype=torch.float32, device="cuda")               # padded rows: ld > V
    pad[:, :V] = _dev(z)
    ops.loo_objective(_dev(z), _dev(y), table, 2)
    ops.loo_objective(pad[:, :V], _dev(y), table, 0)
    got = ops.loo_objective_download(table)
    for slot in (0, 2):
        assert (int(got["right"][slot]), int(got["nan_rows"][slot]), int(got["bad_labels"][slot])) == (want[0], want[2], want[3])
        assert np.float64(got["sum"][slot]).tobytes() == np.float64(want[1]).tobytes(), (got["sum"][slot], want[1])
    assert got["right"][1] == 0 and got["sum"][1] == 0.0     # the slot nobody named keeps its zeros
    if N >= 63:
        assert want[2] == 2 and want[3] == 2 and np.isfinite(want[1])
        right_by_hand = sum(int(np.argmax(z[i]) == y[i]) for i in range(N) if not np.isnan(z[i]).any() and 0 <= y[i] < V)
        assert want[0] == right_by_hand


# ------------------------------------------------------------------------------------------------------- the search ----
FIXTURE_SEED = 0
FIXTURE_V = 6


@functools.lru_cache(maxsize=None)
def fixture_search(scoring):
    """The restatement's search on the N = 60 fixture, and what the comparison with the device rests on: the smallest gap, in
    float32 ulps, between the label's log-prob and the best other class over every evaluated candidate and row, and the largest
    |logp|"""
    X, L, y, codes = ref.make_fixture(FIXTURE_SEED)
    cache, gaps, top = {}, [], []

    def evaluate(w):
        if w not in cache:
            z = ref.loo_logp(X, L, y, FIXTURE_V, codes, w, sum(w)).astype(np.float64)
            lab = z[np.arange(len(y)), y]
            rest = z.copy()
            rest[np.arange(len(y)), y] = -np.inf
            rest = rest.max(axis=1)
            gaps.append(np.min(np.abs(lab - rest) / np.spacing(np.maximum(np.abs(lab), np.abs(rest)).astype(np.float32))))
            top.append(np.abs(z).max())
            cache[w] = ref.loo_objective(z.astype(np.float32), y)[:2]
        return cache[w]
    res = ref.coordinate_search(4, evaluate, levels=(0, 1, 2, 4), sweeps=2, scoring=scoring)
    return dict(res, X=X, L=L, y=y, codes=codes, smallest_gap_ulps=float(min(gaps)), bound=len(y) * 2.0 ** -23 * float(max(top)), evaluate=evaluate)


def _scaled(a, b):
    """Whether one weight vector is a power of two times the other: the same metric with bit-equal votes"""
    return any(tuple(c * v for v in a) == tuple(b) or tuple(c * v for v in b) == tuple(a) for c in (1, 2, 4, 8, 16))


@pytest.mark.parametrize("scoring", ["accuracy", "neg_log_loss"])
def test_fit_field_weights_on_the_fixture(scoring, monkeypatch):
    import slnlp
    from slnlp import ops
    from slnlp.data import TokenDataset
    want = fixture_search(scoring)
    N = len(want["y"])
    # THE CONDITION on the fixture, from the restatement alone: every arg-max decision is clear of the vote's bound (one ulp on
    # either side), and at every step the best candidate leads every other by more than the bound on both sums -- but for a
    # power-of-two multiple of it, which is the same metric with the same bits and loses the tie on W on both sides
    assert want["smallest_gap_ulps"] > 2.0
    if scoring == "neg_log_loss":
        for ranked in want["ranked"]:
            best = ranked[0]
            for other in ranked[1:]:
                assert other[2] - best[2] > 2 * want["bound"] or (_scaled(best[0], other[0]) and other[2] == best[2]), (best, other)
    train = TokenDataset(want["X"], want["L"], want["y"], None)
    downloads = []
    real = ops.loo_objective_download
    monkeypatch.setattr(ops, "loo_objective_download", lambda table: downloads.append(int(table.shape[0])) or real(table))
    got = slnlp.fit_field_weights(train, want["codes"], levels=(0, 1, 2, 4), sweeps=2, scoring=scoring, k=5)
    assert len(got["trace"]) == len(want["trace"]) == got["evaluations"]
    for g, (field, w, right, total) in zip(got["trace"], want["trace"]):
        print(g["field"], g["weights"], g["right"], right, g["sum"], total)
        assert (g["field"], g["weights"]) == (field, w)
        assert g["right"] == right
        assert abs(g["sum"] - total) <= want["bound"]
    assert got["steps"] == want["steps"] and got["weights"] == want["weights"] and got["weights_unreduced"] == want["unreduced"]
    assert got["sweeps_run"] == want["sweeps_run"] and got["converged"] == want["converged"] and got["rows"] == N
    assert downloads == [1] + [len(r) for r in want["ranked"]]              # the start, then ONE download per field step
    start, end = want["trace"][0][2:], want["evaluate"](want["unreduced"])
    if scoring == "accuracy":
        assert want["weights"] == (1, 0, 1, 0) and end[0] > start[0]
        assert got["start_objective"] == start[0] and got["objective"] == end[0] == got["rows_right"]
    else:
        assert end[1] < start[1] and want["weights"][1] == want["weights"][3] == 0 and got["objective"] > got["start_objective"]


# ------------------------------------------------------------------------------------------------------ end to end ----
@functools.lru_cache(maxsize=None)
def _end_to_end_data():
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(400, seq_len=12, src_vocab=64, n_labels=6, seed=5, min_len=3)
    return ds[np.arange(300)], ds[np.arange(300, 400)]


def _end_to_end_table():
    """token v has the parts (v mod 4, (v / 4) mod 4, v / 16)"""
    v = np.arange(64)
    return np.stack([v % 4, (v // 4) % 4, v // 16], axis=1).astype(np.int32)


W3 = (2, 0, 1)


@pytest.fixture(scope="module")
def knn():
    import slnlp
    return slnlp.PhonoKNN(_end_to_end_table(), field_weights=W3, k=5).fit(_end_to_end_data()[0])


def test_estimator_matches_restatement(knn):
    train, test = _end_to_end_data()
    table, S, V = _end_to_end_table(), train.ids.shape[1], len(train.vocab_y)
    assert knn.fields_ == 3 and knn.unit_ == 3 and knn.get_params()["field_weights"] == W3
    dist = ref.distances(test.ids, test.lengths, train.ids, train.lengths, table, W3, 3)
    res = ref.knn_rows(dist, test.lengths, train.lengths, S, S, 5, 3)
    d, i = knn.kneighbors(test)
    assert np.array_equal(d, res["nbr"][:, :, 0]) and np.array_equal(i, res["nbr"][:, :, 1])
    logp, _ = ref.knn_logp(res, test.lengths, train.lengths, train.y, ref.prior_of(train.y, V), 3)
    proba = knn.predict_proba(test)
    want = torch.softmax(torch.from_numpy(logp), dim=-1).numpy()
    assert np.allclose(proba, want, rtol=0, atol=1e-6) and np.array_equal(knn.predict(test), logp.argmax(1))
    assert not np.array_equal(dist, unit_ref.distances(test.ids, test.lengths, train.ids, train.lengths, table, 3))


def test_leave_one_out_reliability_and_compare(knn):
    import slnlp
    train, test = _end_to_end_data()
    table, S = _end_to_end_table(), train.ids.shape[1]
    loo = knn.leave_one_out()
    d, i = loo.kneighbors(train)
    own = ref.distances(train.ids, train.lengths, train.ids, train.lengths, table, W3, 3)
    want = ref.knn_rows(own, train.lengths, train.lengths, S, S, 5, 3, exclude=np.arange(300))
    assert np.array_equal(d, want["nbr"][:, :, 0]) and np.array_equal(i, want["nbr"][:, :, 1]) and (i != np.arange(300)[:, None]).all()
    rel = loo.reliability(train)
    assert rel["rows"] == 300 and np.isfinite([rel["ece"], rel["nll"], rel["accuracy"]]).all() and rel["nan_rows"] == 0
    unit = slnlp.PhonoKNN(table, k=5).fit(train)
    a = unit.compare(knn, test, scoring=["accuracy", "neg_log_loss"], replicates=200, seed=11)
    b = knn.compare(unit, test, scoring=["accuracy", "neg_log_loss"], replicates=200, seed=11)
    for name in ("accuracy", "neg_log_loss"):
        assert a[name]["point"] == pytest.approx(-b[name]["point"]) and a[name]["lower"] == pytest.approx(-b[name]["upper"])
    assert a["neg_log_loss"]["point"] != 0.0


def test_split_audit_in_units_of_W():
    import slnlp
    from slnlp.data import TokenDataset
    train, test = _end_to_end_data()
    table, S = _end_to_end_table(), train.ids.shape[1]
    w = (4, 0, 1)                                            # W = 5
    got = slnlp.split_audit(train, test, radius=5, top=20, field_codes=table, field_weights=w)
    dist = ref.distances(test.ids, test.lengths, train.ids, train.lengths, table, w, 5)
    res = ref.knn_rows(dist, test.lengths, train.lengths, S, S, 1, 5, radius=5)
    assert got["nearest_hist"].shape == (64 * 5 + 2,) and got["rows"] == 100
    assert got["near_duplicates"] == int((res["rows"][:, 1] > 0).sum()) and got["exact_duplicates"] == int((res["nbr"][:, 0, 0] == 0).sum())
    # a row that differs from a train row only in the weight-0 field is an EXACT duplicate at radius 0
    ids = train.ids[7:8].copy()
    assert train.lengths[7] >= 2
    ids[0, 1] ^= 4                                           # (v / 4) mod 4 changes, the other two parts stay
    probe = TokenDataset(ids, train.lengths[7:8], train.y[7:8], train.vocab_X, train.vocab_y)
    exact = slnlp.split_audit(train, probe, radius=0, field_codes=table, field_weights=w)
    assert exact["exact_duplicates"] == 1 and exact["near_duplicates"] == 1 and exact["pairs"][0][2] == 0
    plain = slnlp.split_audit(train, probe, radius=0, field_codes=table)
    assert plain["exact_duplicates"] == 0 and plain["near_duplicates"] == 0


def test_cli_sub_key_writes_its_three_artefacts(tmp_path):
    import json
    from slnlp import cli
    from test_attribution_gpu import make_net
    train, test = _end_to_end_data()
    table = _end_to_end_table()
    torch.manual_seed(9)
    net = make_net(train, max_epochs=1).fit(train)
    opts = cli.phono_baseline_options({"k": 5, "top": 7, "fit_weights": {"sweeps": 1, "scoring": "accuracy"}})
    knn, audit = cli.save_phono_baseline(net, train, test, opts, {"fields": ["orientation", "movement", "handshape"]}, {"replicates": 100},
                                         ["accuracy", "neg_log_loss"], "cuda", str(tmp_path), field_codes=table)
    fit = json.load(open(tmp_path / "train_phono_weights.json"))
    w = fit["weights"]
    assert list(fit["fields"]) == ["orientation", "movement", "handshape"] and list(fit["fields"].values()) == w and len(w) == 3
    assert fit["rows"] == 300 and fit["sweeps_run"] == 1 and fit["evaluations"] == len(fit["trace"]) and fit["scoring"] == "accuracy"
    W = sum(w)
    assert knn.get_params()["field_weights"] == w and knn.unit_ == W
    base = json.load(open(tmp_path / "test_phono_baseline.json"))
    assert base["options"]["field_weights"] == w and base["options"]["unit"] == W and base["options"]["fields"] == 3 and base["options"]["gap"] == W
    assert set(base["phono_vs_weighted"]) >= {"accuracy", "neg_log_loss", "replicates"} and "refit_vs_phono" in base
    assert len(base["neighbours"]["nearest_hist"]) == 64 * W + 2
    split = json.load(open(tmp_path / "test_phono_split_audit.json"))
    assert split["field_weights"] == w and split["radius"] == W and len(split["nearest_hist"]) == 64 * W + 2
    assert split["near_duplicates"] == audit["near_duplicates"] and (tmp_path / "test_phono_split_audit_rows.csv").exists()
