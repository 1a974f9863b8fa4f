"""GPU: edit-distance nearest neighbours on the device -- ``slnlp_edit_distances``, ``slnlp_edit_knn_rows`` and ``slnlp_edit_knn_logp``
through ``slnlp.ops`` against the numpy restatement (tests/edit_knn_ref.py), then ``EditKNN`` and ``split_audit`` end to end.

The bounds.  Distances, neighbours, the per-query rows and the head are integers and EQUAL the restatement's.  The vote is formed
in fp64 in the restatement's order of operations; the device's exp and log may differ from numpy's by an fp64 ulp, which moves the
float32 rounding of log(p) by at most one unit: every finite entry lies within ONE float32 ulp (``np.spacing`` of the restatement's
value) of the restatement, NaN rows match exactly, and the arg-max equals the restatement's wherever its top-two gap exceeds that
ulp.  The tests print how many entries differ at all.

The inputs.  In every case the rows lie S + 3 tokens apart, and the padding and the tokens past a row's length are tokens of the
alphabet both sides draw from, so a read past L changes a distance.  Cases with at least 8 queries and 9 references carry a query
and a reference of lengths 65 and -1, an ``exclude`` list with -1 entries, and duplicated rows (distance 0, index ties)."""
import functools

import numpy as np
import pytest
import torch

import edit_knn_ref as ref

pytestmark = pytest.mark.gpu

RADIUS = 2
#         nq   nr   S   k  alphabet
SHAPES = [(1, 1, 1, 1, "small"),          # the smallest case
          (3, 2, 5, 4, "small"),          # k > nr: found < k, the (-1, -1) tail
          (5, 7, 63, 3, "small"),         # lengths 0, 1, 62 and 63 on both sides
          (8, 9, 64, 5, "small"),         # 0, 1, 63 and 64: the top bit of the word
          (65, 257, 48, 5, "wide"),       # more references than one block's threads, queries past a wave
          (257, 300, 64, 64, "three"),    # an alphabet of 3 tokens: almost every distance tied, k at its cap
          (33, 40, 17, 5, "high")]        # tokens that differ only above bit 32: a 32-bit compare shows
IDS = [f"{nq}x{nr}x{S}k{k}" for nq, nr, S, k, _ in SHAPES]
ALPHABETS = {"small": np.arange(2, 8), "wide": np.arange(2, 40), "three": np.arange(5, 8),
             "high": (np.arange(1, 5, dtype=np.int64) << 33) + 7}          # 2^33 t + 7: equal in their low 32 bits


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _lengths(rs, n, S):
    """random ones, then S, 0, S - 1 and 1 in the last places (as far as n goes): the rows a case rewrites are the first six"""
    edge = np.array([S, 0, S - 1, 1], dtype=np.int64)[:n]
    return np.concatenate([rs.randint(0, S + 1, size=n - len(edge)), edge]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(index):
    """One shape's inputs and the restatement's outputs, formed once and shared (nobody writes to them)"""
    nq, nr, S, k, name = SHAPES[index]
    rs = np.random.RandomState(100 + index)
    alphabet = ALPHABETS[name]
    token = lambda m: rs.choice(alphabet, size=m)
    Xq, Lq = ref.make_rows(rs, nq, S, alphabet, _lengths(rs, nq, S), token)
    Xr, Lr = ref.make_rows(rs, nr, S, alphabet, _lengths(rs, nr, S), token)
    exclude = None
    if nq >= 8 and nr >= 9:
        Lr[0] = S if S >= 63 else max(Lr[0], min(S, 3))      # S = 64: two identical rows of 64 tokens, bit 63 all the way
        Xr[0, :Lr[0]] = token(Lr[0])
        Xr[5], Lr[5] = Xr[0], Lr[0]                          # a duplicated reference, and a query that equals both
        Xq[0], Lq[0] = Xr[0], Lr[0]
        Xq[4, :min(Lq[4], Lr[6])] = Xr[6, :min(Lq[4], Lr[6])]
        Lq[1], Lq[3], Lr[2], Lr[4] = 65, -1, 65, -1
        exclude = np.where(rs.rand(nq) < 0.5, -1, rs.randint(0, nr, size=nq)).astype(np.int64)
        exclude[0], exclude[2] = 0, -1                       # query 0 skips its twin 0 and finds the copy 5
    dist = ref.distances(Xq, Lq, Xr, Lr)
    res = ref.knn_rows(dist, Lq, Lr, S + 3, S + 3, k, radius=RADIUS, exclude=exclude)
    return dict(nq=nq, nr=nr, S=S, k=k, Xq=Xq, Lq=Lq, Xr=Xr, Lr=Lr, exclude=exclude, dist=dist, res=res)


def _device_rows(c):
    """The rows as the device sees them: [n, S] views of tensors whose rows lie S + 3 apart"""
    S = c["S"]
    return _dev(c["Xq"])[:, :S], _dev(c["Lq"]), _dev(c["Xr"])[:, :S], _dev(c["Lr"])


def _search(c, sl=slice(None)):
    from slnlp import ops
    Xq, Lq, Xr, Lr = _device_rows(c)
    ex = None if c["exclude"] is None else _dev(c["exclude"])[sl]
    return ops.edit_knn_rows(Xq[sl], Lq[sl], Xr, Lr, c["k"], radius=RADIUS, exclude=ex)


# ---------------------------------------------------------------------------------------------------------- integers ----
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=IDS)
def test_distances_equal_restatement(index):
    from slnlp import ops
    c = case(index)
    got = ops.edit_distances(*_device_rows(c)).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (c["nq"], c["nr"])
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


def test_ties_dominate_the_large_case():
    c = case(5)
    kth = c["res"]["nbr"][:, c["k"] - 1, 0]
    tied = [(c["dist"][i] == kth[i]).sum() > 1 for i in range(c["nq"]) if kth[i] >= 0]
    assert np.mean(tied) > 0.9


# ------------------------------------------------------------------------------------------------------------- votes ----
@pytest.mark.parametrize("weights", ["uniform", "distance"])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("index,V", [(3, 7), (4, 70), (5, 7)], ids=["8x9", "65x257", "257x300"])
def test_votes_within_one_float32_ulp(index, V, normalize, weights):
    from slnlp import ops
    c = case(index)
    rs = np.random.RandomState(7 + index)
    yr = rs.randint(0, V, size=c["nr"]).astype(np.int64)
    yr[1], yr[3] = -1, V                                     # labels outside the classes: skipped and counted
    prior = ref.prior_of(yr[(yr >= 0) & (yr < V)], V)
    tau, lam = 0.75, 0.5
    want, bad = ref.knn_logp(c["res"], c["Lq"], c["Lr"], yr, prior, weights=weights, tau=tau, normalize=normalize, lam=lam)
    buf = _search(c)
    out = torch.full((c["nq"], V + 3), 7.0, dtype=torch.float32, device="cuda")          # padded rows: the padding stays
    ops.edit_knn_logp(buf, _dev(c["Lq"]), _dev(c["Lr"]), _dev(yr), _dev(prior), weights=weights, tau=tau, normalize=normalize, lam=lam,
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


def test_found_zero_is_the_log_prior():
    from slnlp import ops
    c = case(0)                                              # one query, one reference, excluded: no neighbour
    Xq, Lq, Xr, Lr = _device_rows(c)
    buf = ops.edit_knn_rows(Xq, Lq, Xr, Lr, 1, exclude=_dev(np.zeros(1, dtype=np.int64)))
    prior = np.array([0.2, 0.5, 0.3])
    got = ops.edit_knn_logp(buf, Lq, Lr, _dev(np.zeros(1, dtype=np.int64)), _dev(prior), lam=2.0).cpu().numpy()
    assert ops.edit_knn_download(buf)["rows"][0, 0] == 0
    want = np.log((2.0 * prior) / 2.0).astype(np.float32)
    assert (np.abs(got[0] - want) <= np.spacing(np.abs(want))).all()


# ------------------------------------------------------------------------------------------------------ equal bytes ----
def test_equal_bytes_across_runs_and_chunks():
    from slnlp import ops
    c = case(4)
    yr = _dev(np.random.RandomState(3).randint(0, 9, size=c["nr"]).astype(np.int64))
    prior = _dev(np.full(9, 1.0 / 9))

    def run(sl=slice(None)):
        buf = _search(c, sl)
        z = ops.edit_knn_logp(buf, _dev(c["Lq"])[sl], _dev(c["Lr"]), yr, prior)
        got = ops.edit_knn_download(buf)
        return got["rows"].copy(), got["nbr"].copy(), z.cpu().numpy()
    a, b = run(), run()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                            # another stream: the same bytes
        s = run()
    side.synchronize()
    parts = [run(slice(0, 7)), run(slice(7, 40)), run(slice(40, None))]
    for i in range(3):
        assert a[i].tobytes() == b[i].tobytes() == s[i].tobytes()
        assert a[i].tobytes() == np.concatenate([p[i] for p in parts]).tobytes()


def test_library_refusals():
    from slnlp import ops
    c = case(2)
    Xq, Lq, Xr, Lr = _device_rows(c)
    with pytest.raises(ValueError, match="edit_knn_rows: k=65"):
        ops.edit_knn_rows(Xq, Lq, Xr, Lr, 65)
    with pytest.raises(ValueError, match="edit_knn_rows: exclude must be"):
        ops.edit_knn_rows(Xq, Lq, Xr, Lr, 2, exclude=_dev(np.zeros(3, dtype=np.int64)))
    with pytest.raises(ValueError, match="edit_distances: the query rows must be"):
        ops.edit_distances(Xq.int(), Lq, Xr, Lr)
    with pytest.raises(RuntimeError, match="scratch of 3 bytes is too small"):
        ops.edit_knn_rows(Xq, Lq, Xr, Lr, 2, scratch=torch.empty(3, dtype=torch.uint8, device="cuda"))
    buf = ops.edit_knn_rows(Xq, Lq, Xr, Lr, 2)
    with pytest.raises(RuntimeError, match="output head overlaps input prior"):
        ops.edit_knn_logp(buf, Lq, Lr, Lr, buf["head"].view(torch.float64)[:4])


# ------------------------------------------------------------------------------------------------------ end to end ----
@pytest.fixture(scope="module")
def data():
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(400, seq_len=12, src_vocab=64, n_labels=6, seed=5, min_len=3)
    return ds[np.arange(300)], ds[np.arange(300, 400)]


@pytest.fixture(scope="module")
def expected(data):
    """The restatement on the end-to-end data: distances, the 5 neighbours, EditKNN's default vote"""
    train, test = data
    V, S = len(train.vocab_y), train.ids.shape[1]
    dist = ref.distances(test.ids, test.lengths, train.ids, train.lengths)
    res = ref.knn_rows(dist, test.lengths, train.lengths, S, S, 5)
    logp, _ = ref.knn_logp(res, test.lengths, train.lengths, train.y, ref.prior_of(train.y, V))
    one, _ = ref.knn_logp(ref.knn_rows(dist, test.lengths, train.lengths, S, S, 1), test.lengths, train.lengths, train.y, ref.prior_of(train.y, V))
    return dict(dist=dist, res=res, logp=logp, one=one)


@pytest.fixture(scope="module")
def knn(data):
    import slnlp
    return slnlp.EditKNN(k=5).fit(data[0])


def test_estimator_matches_restatement(data, expected, knn):
    import slnlp
    train, test = data
    d, i = knn.kneighbors(test)
    assert d.dtype == np.int32 and i.dtype == np.int64
    assert np.array_equal(d, expected["res"]["nbr"][:, :, 0]) and np.array_equal(i, expected["res"]["nbr"][:, :, 1])
    d3, i3 = knn.kneighbors(test, k=3)
    assert np.array_equal(d3, d[:, :3]) and np.array_equal(i3, i[:, :3])
    proba = knn.predict_proba(test)
    want = torch.softmax(torch.from_numpy(expected["logp"]), dim=-1).numpy()
    assert np.allclose(proba, want, rtol=0, atol=1e-6) and np.allclose(proba.sum(1), 1.0, atol=1e-5)
    pred = knn.predict(test)
    assert np.array_equal(pred, expected["logp"].argmax(1))
    assert round(float((pred == test.y).mean()), 2) == 0.57 and knn.score(test) == pytest.approx(0.57)
    one = slnlp.EditKNN(k=1).fit(train).predict(test)
    assert np.array_equal(one, expected["one"].argmax(1)) and round(float((one == test.y).mean()), 2) == 0.53
    assert np.array_equal(knn.classes_, np.arange(len(train.vocab_y))) and knn.prior_.sum() == pytest.approx(1.0)


def test_chunked_queries_give_the_same_bytes(data, knn):
    import copy
    _, test = data
    whole = knn._forward_logp(test, lambda z, y: z.cpu().numpy())
    small = copy.copy(knn)
    small._cap = 300 * 7                                     # 7 queries per chunk: 15 chunks, the last of 2
    assert whole.tobytes() == small._forward_logp(test, lambda z, y: z.cpu().numpy()).tobytes()
    assert np.array_equal(knn.kneighbors(test)[1], small.kneighbors(test)[1])


def test_leave_one_out(data, knn):
    import slnlp
    from slnlp.data import TokenDataset
    train, test = data
    loo = knn.leave_one_out()
    d, i = loo.kneighbors(train)
    assert (i != np.arange(len(train))[:, None]).all() and (i >= 0).all()
    with pytest.raises(ValueError, match="leave-one-out log-probs exist only for the 300 rows"):
        loo.predict(test)
    twice = TokenDataset(np.concatenate([train.ids, train.ids[7:8]]), np.concatenate([train.lengths, train.lengths[7:8]]),
                         np.concatenate([train.y, train.y[7:8]]), train.vocab_X, train.vocab_y)
    d2, i2 = slnlp.EditKNN(k=2).fit(twice).leave_one_out().kneighbors(twice)
    assert (d2[7, 0], i2[7, 0]) == (0, 300) and (d2[300, 0], i2[300, 0]) == (0, 7)
    rel = loo.reliability(train)
    assert rel["rows"] == 300 and np.isfinite([rel["ece"], rel["nll"], rel["accuracy"]]).all() and rel["nan_rows"] == 0
    issues = loo.label_issues(train)
    assert len(issues["issues"]["row"]) <= 300
    assert np.isfinite(loo.ranking(train)["auc_macro"])
    ci = loo.score_interval(train, scoring="accuracy", replicates=100, seed=1)
    assert ci["accuracy"]["point"] == pytest.approx(rel["accuracy"]) and ci["rows"] == 300
    with pytest.raises(NotImplementedError, match="leave-one-out"):
        loo.attribute(train)


def test_diagnostics_run_on_the_baseline(data, knn):
    _, test = data
    rel = knn.reliability(test)
    assert rel["accuracy"] == pytest.approx(0.57) and np.isfinite([rel["ece"], rel["mce"], rel["brier"], rel["nll"]]).all()
    rank = knn.ranking(test)
    assert np.isfinite(rank["auc_macro"]) and rank["auc_macro"] > 0.5
    labels, proba = knn.predict_topk(test, k=3)
    assert np.array_equal(labels[:, 0], knn.predict(test)) and np.isfinite(proba).all()
    ci = knn.score_interval(test, scoring=["accuracy", "neg_log_loss"], replicates=200, seed=3)
    assert ci["accuracy"]["point"] == pytest.approx(0.57) and ci["accuracy"]["lower"] <= 0.57 <= ci["accuracy"]["upper"]
    assert np.isfinite([ci["neg_log_loss"]["point"], ci["neg_log_loss"]["lower"], ci["neg_log_loss"]["upper"]]).all()
    att = knn.attribute(test, by="frame")
    assert att["rows"] == 100 and np.isfinite(att["top_drop"]).all() and att["usable"] == int(test.lengths.sum())


@pytest.fixture(scope="module")
def net(data):
    """One tiny fused fit: a one-epoch GRU"""
    from test_attribution_gpu import make_net
    torch.manual_seed(9)
    return make_net(data[0], max_epochs=1).fit(data[0])


def test_compare_with_a_fit(data, knn, net):
    train, test = data
    a = net.compare(knn, test, scoring=["accuracy", "neg_log_loss"], replicates=200, seed=11)
    b = knn.compare(net, test, scoring=["accuracy", "neg_log_loss"], replicates=200, seed=11)
    for name in ("accuracy", "neg_log_loss"):
        assert a[name]["point"] == pytest.approx(-b[name]["point"]) and a[name]["mean"] == pytest.approx(-b[name]["mean"])
        assert a[name]["lower"] == pytest.approx(-b[name]["upper"])
    assert a["neg_log_loss"]["point"] != 0.0


def test_split_audit(data, expected, knn):
    import slnlp
    from slnlp import metrics
    train, test = data
    S = train.ids.shape[1]
    got = slnlp.split_audit(train, test, radius=4, top=20, judge=knn)
    res = ref.knn_rows(expected["dist"], test.lengths, train.lengths, S, S, 1, radius=4)
    want = metrics.split_audit_report(res["rows"], res["nbr"], test.y, train.y, 4, 20, head=res["head"])
    for key in ("rows", "exact_duplicates", "near_duplicates", "conflicting", "conflicting_exact", "pairs", "flagged_queries", "flagged_references"):
        assert got[key] == want[key], key
    assert np.array_equal(got["nearest_hist"], want["nearest_hist"]) and np.array_equal(got["duplicated"], want["duplicated"])
    for key in ("label", "support", "duplicated", "conflicting"):
        assert np.array_equal(got["per_class"][key], want["per_class"][key])
    assert got["near_duplicates"] > 0 and got["self"] is False
    right = knn.predict(test) == test.y
    dup = want["duplicated"]
    assert got["rows_duplicated"] == dup.sum() and got["rows_clean"] == (~dup).sum()
    assert got["accuracy_duplicated"] == pytest.approx(right[dup].mean()) and got["accuracy_clean"] == pytest.approx(right[~dup].mean())
    own = slnlp.split_audit(train, train, radius=4)
    loo = ref.knn_rows(ref.distances(train.ids, train.lengths, train.ids, train.lengths), train.lengths, train.lengths, S, S, 1, radius=4,
                       exclude=np.arange(300))
    assert own["self"] is True and own["near_duplicates"] == int((loo["rows"][:, 2] <= 4).sum()) and all(q != r for q, r, *_ in own["pairs"])


def test_cli_baseline_files(data, net, tmp_path):
    import csv
    import json
    from slnlp import cli
    train, test = data
    opts = cli.baseline_options({"k": 5, "radius": 4, "top": 7})
    knn, audit = cli.save_baseline(net, train, test, opts, {"replicates": 100}, ["accuracy", "neg_log_loss"], "cuda", str(tmp_path))
    base = json.load(open(tmp_path / "test_baseline.json"))
    assert base["scores"]["test_accuracy"] == pytest.approx(0.57) and np.isfinite(base["scores"]["test_neg_log_loss"])
    assert base["options"]["k"] == 5 and base["train_rows"] == 300 and base["neighbours"]["rows"] == 100
    assert set(base["refit_vs_baseline"]) >= {"accuracy", "neg_log_loss", "replicates"}
    split = json.load(open(tmp_path / "test_split_audit.json"))
    assert split["rows"] == 100 and split["near_duplicates"] == audit["near_duplicates"] and len(split["pairs"]) == 7 and len(split["nearest_hist"]) == 66
    assert split["rows_duplicated"] + split["rows_clean"] == 100
    lines = list(csv.reader(open(tmp_path / "test_split_audit_rows.csv")))
    assert lines[0][:4] == ["row", "label", "name", "nearest"] and len(lines) == 101
    assert sum(int(r[7]) for r in lines[1:]) == split["near_duplicates"]
