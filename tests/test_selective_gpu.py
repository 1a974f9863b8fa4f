"""GPU: selective prediction on the device -- ``slnlp_selective_rows`` / ``_counts`` through the C ABI against the numpy restatement
(tests/selective_ref.py), ``NeuralNetClassifier.risk_coverage`` / ``fit_rejection`` / ``predict_selective`` and the two wrappers'.

The bounds.  pred, wrong, code, the counts and the level results are integers and equal the restatement's; ``accepted`` is compared
at a threshold that every restated kappa stays more than 1e-9 away from, which the test checks as a condition on the inputs.
max_prob and margin are probabilities from the shared row head: within the project's 1e-12 absolute; neg_entropy is a sum of at
most 1024 terms of magnitude <= ln 1024, each a few 2^-53 off in relative terms: within 1e-12 ln 1024.  AURC is a mean of n terms
<= 1, each correctly rounded, added in some fixed order: within 2 n 2^-53 of the restatement's ``math.fsum``.  The tests print the
measured maxima; DESIGN.md section 4 records them."""
import math
import warnings

import numpy as np
import pytest
import torch

import conformal_ref as cr
import selective_ref as sr

pytestmark = pytest.mark.gpu

BOUND = {"max_prob": 1e-12, "margin": 1e-12, "neg_entropy": 1e-12 * math.log(1024.0)}
MARGIN = 1e-9
RISKS, COVERAGES = [0.0, 0.01, 0.05, 0.1, 0.5, 1.0], [0.0, 0.25, 0.5, 0.8, 0.9, 0.999, 1.0]


def _device(z, y=None, ld=None):
    """``z`` on the device, its rows ``ld`` floats apart (the padding is NaN: never to be read), and the labels."""
    N, V = z.shape
    buf = torch.full((N, ld or V), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(z).cuda()
    return buf[:, :V], (None if y is None else torch.from_numpy(np.asarray(y, dtype=np.int64)).cuda())


def _state(tau):
    return torch.tensor([tau, 0.0, 0.0, 0.0], dtype=torch.float64).cuda()


def _pick_tau(kappa):
    """A threshold near the median of the finite ``kappa`` that none of them comes closer to than MARGIN: the midpoint of the
    widest gap between neighbouring values around the median (below the single value when there is only one)."""
    v = np.unique(kappa[np.isfinite(kappa)])
    if v.size < 2:
        return float(v[0] - 0.25) if v.size else 0.5
    i = v.size // 2
    lo, hi = max(0, i - 8), min(v.size - 1, i + 8)
    g = int(np.argmax(np.diff(v[lo:hi + 1])))
    return float(0.5 * (v[lo + g] + v[lo + g + 1]))


def _special():
    z, y = cr.make_logp(12, 9, 8)
    z[0] = -np.inf
    z[0, 4] = 0.0                                                                # p = 1 and the rest -inf: 0 * -inf must not appear
    y[0] = 4
    z[1, 3] = -np.inf                                                            # -inf: an ordinary value, p = 0
    y[1] = 3
    z[2, 6] = np.nan                                                             # code -2
    z[3, 0] = np.inf                                                             # code -2: the maximum is not finite
    z[4, 2], z[4, 5] = -0.0, 0.0                                                 # equal values: by ascending column
    z[5] = -np.inf                                                               # code -2: the maximum is -inf
    z[6, 1] = z[6, 7] = z[6].max() + 1.0                                         # two columns at the maximum: margin 0
    return z, y


def _bad_labels():
    z, y = cr.make_logp(20, 6, 6)
    y[3], y[10], y[19] = -1, 6, 2 ** 40
    z[10, 1] = np.nan                                                            # a NaN row with a bad label: the NaN is looked at first
    return z, y


def _row_cases():
    return [("N1_V1", np.zeros((1, 1), dtype=np.float32), np.array([0]), None, 1.0),
            ("N5_V3", *cr.make_logp(5, 3, 1), None, 1.0),
            ("N70_V63", *cr.make_logp(70, 63, 2), None, 1.0),                    # one short of a wave
            ("N70_V64", *cr.make_logp(70, 64, 3), None, 1.0),
            ("N70_V65", *cr.make_logp(70, 65, 4), None, 1.0),
            ("N300_V202", *cr.make_logp(300, 202, 5), None, 1.0),
            ("N33_V129_ld136", *cr.make_logp(33, 129, 6), 136, 1.0),
            ("N64_V70_ties", *cr.make_logp(64, 70, 7, quantum=0.25), None, 1.0), # equal maxima
            ("special_rows", *_special(), None, 1.0),
            ("bad_labels", *_bad_labels(), None, 1.0),
            ("beta_0.5", *cr.make_logp(70, 33, 9), None, 0.5),
            ("beta_2.0", *cr.make_logp(70, 33, 10, quantum=0.25), None, 2.0)]


@pytest.mark.parametrize("case", _row_cases(), ids=lambda c: c[0])
def test_rows_kernel_against_the_restatement(case):
    from slnlp import ops
    name, z, y, ld, beta = case
    N, V = z.shape
    zd, yd = _device(z, y, ld)
    if ld:
        assert zd.stride(0) == ld > V
    state = ops.temperature_state(beta, "cuda") if beta != 1.0 else None
    for score in sr.SCORES:
        free = sr.rows_ref(z, y, beta=beta, score=score)
        tau = _pick_tau(free["kappa"])
        want = sr.rows_ref(z, y, beta=beta, score=score, tau=tau)
        ok = np.isfinite(want["kappa"])
        assert not ok.any() or np.abs(want["kappa"][ok] - tau).min() > MARGIN, (name, score)      # a condition on the inputs
        got = ops.selective_download(ops.selective_rows(zd, yd, score=score, state=state, tau=_state(tau)), counts=False)
        assert got["rows"].dtype == np.int32 and np.array_equal(got["rows"], want["rows"]), \
            (name, score, np.flatnonzero((got["rows"] != want["rows"]).any(axis=1))[:8])
        assert np.array_equal(np.isnan(got["kappa"]), np.isnan(want["kappa"])) and np.array_equal(np.isnan(got["kappa"]), want["rows"][:, 3] == -2)
        err = float(np.abs(got["kappa"][ok] - want["kappa"][ok]).max()) if ok.any() else 0.0
        print(f"{name} {score}: max |kappa - restatement| = {err:.3e} (bound {BOUND[score]:.3e}), tau {tau:.6f}, "
              f"accepted {int(want['rows'][:, 2].sum())} of {N}")
        assert err <= BOUND[score], (name, score, err)
        # without a threshold nothing is accepted; without labels nothing is wrong and no code is -1; the rest keeps its bits
        bare = ops.selective_download(ops.selective_rows(zd, yd, score=score, state=state), counts=False)
        assert bare["kappa"].tobytes() == got["kappa"].tobytes() and np.array_equal(bare["rows"][:, [0, 1, 3]], got["rows"][:, [0, 1, 3]])
        assert not bare["rows"][:, 2].any()
        blind = ops.selective_download(ops.selective_rows(zd, None, score=score, state=state, tau=_state(tau)), counts=False)
        assert blind["kappa"].tobytes() == got["kappa"].tobytes() and np.array_equal(blind["rows"][:, [0, 2]], got["rows"][:, [0, 2]])
        assert not blind["rows"][:, 1].any() and set(blind["rows"][:, 3]) <= {0, -2}
        if score == "max_prob":                                                  # the same statements as topk_rows: the same bits
            top = ops.topk_download(ops.topk_rows(zd, 1, state=state))
            assert got["kappa"].tobytes() == top[1][:, 0].tobytes() and np.array_equal(got["rows"][:, 0], top[0][:, 0])
    if name == "special_rows":
        assert want["rows"][[2, 3, 5], 3].tolist() == [-2, -2, -2] and sr.rows_ref(z, y, score="margin")["kappa"][6] == 0.0
        assert sr.rows_ref(z, y, score="neg_entropy")["kappa"][0] == 0.0 and sr.rows_ref(z, y, score="max_prob")["kappa"][0] == 1.0
    if name == "bad_labels":
        assert want["rows"][[3, 10, 19], 3].tolist() == [-1, -2, -1] and not want["rows"][[3, 10, 19], 1].any()
    if name == "N1_V1":
        assert [sr.rows_ref(z, y, score=s)["kappa"][0] for s in sr.SCORES] == [1.0, 1.0, 0.0]


# --------------------------------------------------------------------------------------------------------- counts ----
def _feed(kappa, rows, risks=RISKS, coverages=COVERAGES, poison=True):
    """The counts kernel on arrays given directly (so ties are exact): ``ops.selective_download``'s dict."""
    from slnlp import ops
    buf = ops.selective_buffers(len(kappa), "cuda")
    if poison:
        buf["flat"].view(torch.int64).fill_(0x7F7F7F7F7F7F7F7F)
    buf["kappa"].copy_(torch.from_numpy(np.ascontiguousarray(kappa)))
    buf["rows"].copy_(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)))
    assert ops.selective_counts(buf, risks, coverages) is buf["table"]
    return ops.selective_download(buf)


def _check_counts(name, kappa, rows, risks=RISKS, coverages=COVERAGES):
    got = _feed(kappa, rows, risks, coverages)
    table, want = sr.table_ref(kappa, rows, risks, coverages)
    n = want["n"]
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], want["counts"]), \
        (name, np.flatnonzero((got["counts"] != want["counts"]).any(axis=1))[:8])
    assert got["table"].shape == table.shape and got["table"][:4].tolist() == table[:4].tolist(), (name, got["table"][:8])
    assert got["table"][6:8].tolist() == [0.0, 0.0]
    assert np.array_equal(got["table"][8:sr.HEAD], table[8:sr.HEAD]), (name, got["table"][8:sr.HEAD], table[8:sr.HEAD])      # the levels: exact
    bound = 2 * max(n, 1) * 2.0 ** -53
    if n:
        err = abs(got["table"][5] - want["aurc"])
        print(f"{name}: n {n}, E {want['E']}, AURC {got['table'][5]:.6f}, |AURC - fsum| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (name, err)
        assert abs(got["table"][4] - want["risk_sum"]) <= n * bound and got["table"][5] == got["table"][4] / n
        assert np.abs(got["table"][sr.HEAD:] - table[sr.HEAD:]).max() <= sr.CHUNK * bound          # the chunk sums, zeros behind the last chunk
        assert not got["table"][sr.HEAD + (n + sr.CHUNK - 1) // sr.CHUNK:].any()
    else:
        assert math.isnan(got["table"][5]) and got["table"][4] == 0.0 and not got["table"][sr.HEAD:].any()
    return got


SIZES = [1, 2, 2047, 2048, 2049, 4099]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", ["distinct", "tied", "levels8"])
def test_counts_kernel_against_the_restatement(N, kind):
    kappa, rows = sr.make_counts_case(N, 100 + N, levels={"distinct": None, "tied": 1, "levels8": 8}[kind])
    if kind == "distinct":
        assert len(np.unique(kappa)) == N
    _check_counts(f"N{N}_{kind}", kappa, rows)


def _excluded_run_at_the_start():
    kappa, rows = sr.make_counts_case(2100 + 2500, 31, levels=8)
    rows[:2100, 3] = np.where(np.arange(2100) % 2 == 0, -1, -2)                  # more than a chunk of excluded rows first:
    rows[:2100, 1] = 0                                                           # the chunks go by included ordinal, not by row
    kappa[:2100:2] = 0.5                                                         # a code -1 row keeps a kappa, which must not count
    kappa[1:2100:2] = np.nan
    return kappa, rows


def _signed_zeros():
    kappa, rows = sr.make_counts_case(600, 32, levels=4, signed=True, excluded=0.05)
    zero = np.flatnonzero(kappa == 0.0)
    kappa[zero[::2]] = -0.0
    assert np.signbit(kappa[zero]).any() and not np.signbit(kappa[zero]).all() and (kappa < 0).any()
    return kappa, rows


def _nan_with_code_0():
    kappa, rows = sr.make_counts_case(300, 33, excluded=0.1)
    kappa[5], kappa[17] = np.nan, np.nan                                         # counted with the -2 rows whatever the code says
    rows[5, 3], rows[17, 3] = 0, 0
    return kappa, rows


@pytest.mark.parametrize("case", [("no_errors", *sr.make_counts_case(2500, 21, levels=8, error_rate=0.0)),
                                  ("all_errors", *sr.make_counts_case(2500, 22, levels=8, error_rate=1.0)),
                                  ("excluded_interleaved", *sr.make_counts_case(4099, 23, levels=8, excluded=0.3)),
                                  ("excluded_interleaved_distinct", *sr.make_counts_case(3000, 24, excluded=0.5)),
                                  ("excluded_run_at_the_start", *_excluded_run_at_the_start()),
                                  ("all_excluded", np.full(70, np.nan), np.tile(np.array([[0, 0, 0, -2]], dtype=np.int32), (70, 1))),
                                  ("signed_zeros", *_signed_zeros()),
                                  ("nan_with_code_0", *_nan_with_code_0()),
                                  ("infinite_kappa", np.array([np.inf, 1.0, -np.inf, np.inf, 0.0]), np.array([[0, 0, 0, 0], [0, 1, 0, 0]] * 2 + [[0, 0, 0, 0]]))],
                         ids=lambda c: c[0])
def test_counts_kernel_edge_cases(case):
    name, kappa, rows = case
    got = _check_counts(name, kappa, rows)
    if name == "no_errors":
        assert got["table"][1] == 0 and got["table"][5] == 0.0 and got["table"][8:10].tolist() == [2500.0, 0.0]       # risk 0: everything
    if name == "all_errors":
        assert got["table"][1] == 2500 and got["table"][5] == 1.0 and not got["table"][8:18].any() and got["table"][18:20].tolist() == [2500.0, 2500.0]
    if name == "excluded_run_at_the_start":
        assert got["table"][:4].tolist() == [2500.0, got["table"][1], 1050.0, 1050.0] and not got["counts"][:2100].any()
    if name == "nan_with_code_0":
        assert not got["counts"][[5, 17]].any()
    if name == "all_excluded":
        assert got["table"][:4].tolist() == [0.0, 0.0, 0.0, 70.0] and not got["table"][8:sr.HEAD].any()


def test_no_levels_and_eight_levels():
    kappa, rows = sr.make_counts_case(700, 41, levels=16)
    none = _check_counts("no_levels", kappa, rows, [], [])
    assert not none["table"][8:sr.HEAD].any()
    eight = _check_counts("eight_levels", kappa, rows, list(np.linspace(0.0, 0.7, 8)), list(np.linspace(0.05, 1.0, 8)))
    assert eight["table"][8 + 2 * 7] == 700.0 and eight["table"][24 + 2 * 7] == 700.0       # risk 0.7 and coverage 1.0: every row


def test_counts_are_a_pure_function_of_the_arguments():
    kappa, rows = sr.make_counts_case(4099, 51, levels=8, excluded=0.1)
    a = _feed(kappa, rows)
    b = _feed(kappa, rows, poison=False)
    for key in ("table", "kappa", "rows", "counts"):
        assert a[key].tobytes() == b[key].tobytes(), key
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = _feed(kappa, rows)
    side.synchronize()
    assert c["table"].tobytes() == a["table"].tobytes() and c["counts"].tobytes() == a["counts"].tobytes()
    # permuting the rows permutes the counts; n, E, the levels are those of the multiset (the sum is added in another order)
    p = np.random.RandomState(1).permutation(4099)
    d = _feed(kappa[p], rows[p])
    assert np.array_equal(d["counts"], a["counts"][p]) and np.array_equal(d["table"][:4], a["table"][:4])
    assert np.array_equal(d["table"][8:sr.HEAD], a["table"][8:sr.HEAD]) and abs(d["table"][5] - a["table"][5]) <= 2 * 4099 * 2.0 ** -53


def test_rows_then_counts_and_one_download(monkeypatch):
    from slnlp import metrics, ops
    z, y = cr.make_logp(300, 37, 14, lean=3.0)                                   # 51 of 300 wrong: a risk of 0.1 is within reach
    zd, yd = _device(z, y)
    buf = ops.selective_rows(zd, yd, score="margin")
    ops.selective_counts(buf, [0.1], [0.9])
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(t.numel() * t.element_size()) or real(t, *a, **k))
    got = ops.selective_download(buf)
    monkeypatch.undo()
    assert len(copies) == 1 and copies[0] <= (sr.HEAD + 1) * 8 + 300 * 32 + 8, copies      # one copy: the table, 32 bytes a row, at most a pad
    table, want = sr.table_ref(got["kappa"], got["rows"], [0.1], [0.9])          # fed the device's own kappa
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["table"][8:sr.HEAD], table[8:sr.HEAD])
    rep = metrics.selective_report(got["kappa"], got["rows"], got["counts"], got["table"], got["risks"], got["coverages"])
    assert rep["rows"] == 300 and rep["errors"] == int((z.argmax(axis=1) != y).sum()) and rep["e_aurc"] >= -1e-15
    assert rep["coverage_at_risk"][0]["accepted"] > 0 and rep["coverage_at_risk"][0]["selective_risk"] <= 0.1
    assert rep["risk_at_coverage"][0]["achieved_coverage"] >= 0.9


def test_bad_arguments_return_codes_and_messages():
    import ctypes as C

    from slnlp import _lib, ops
    lib = _lib.load()
    z, y = _device(*cr.make_logp(5, 3, 1))
    buf = ops.selective_buffers(5, "cuda")
    tau, beta = _state(0.5), ops.temperature_state(1.0, "cuda")
    p, st = _lib.ptr, _lib.stream_ptr()
    call = lambda *a: (lib.slnlp_selective_rows(*a, st), lib.slnlp_last_error().decode())
    #       0     1   2     3  4  5  6        7       8                 9
    good = (p(z), 3, p(y), 5, 3, 0, p(beta), p(tau), p(buf["kappa"]), p(buf["rows"]))
    assert call(*good)[0] == 0
    for i, value, text in [(0, None, "null pointer"), (8, None, "null pointer"), (9, None, "null pointer"), (3, 0, "N=0"),
                           (3, 1048577, "N=1048577"), (4, 0, "V=0"), (4, 2 ** 31 - 1, "V=2147483647"), (1, 2, "ld=2 is less than V=3"),
                           (1, 2 ** 62, "is no addressable matrix"), (5, 3, "score=3"), (5, -1, "score=-1"),
                           (0, p(z) + 2, "misaligned"), (2, p(y) + 4, "misaligned"), (6, p(beta) + 4, "misaligned"), (7, p(tau) + 4, "misaligned"),
                           (8, p(buf["kappa"]) + 4, "misaligned"), (9, p(buf["rows"]) + 8, "16-byte aligned"),
                           (9, p(buf["kappa"]) + (-p(buf["kappa"]) % 16), "outputs kappa and rows overlap")]:
        args = list(good)
        args[i] = value
        rc, msg = call(*args)
        assert rc == 1 and "selective_rows" in msg and text in msg, (i, value, rc, msg)
    big = torch.zeros(64, dtype=torch.float64, device="cuda")                    # an output over an input: nothing is launched
    for i, o, text in [(0, 8, "output kappa overlaps input logp"), (2, 9, "output rows overlaps input y"),
                       (6, 8, "output kappa overlaps input beta"), (7, 9, "output rows overlaps input tau")]:
        args = list(good)
        args[i], args[o] = p(big), p(big)
        rc, msg = call(*args)
        assert rc == 1 and text in msg, (i, o, rc, msg)
    for drop in [(2,), (6,), (7,), (2, 6, 7)]:                                   # what may be null
        args = list(good)
        for i in drop:
            args[i] = None
        assert call(*args)[0] == 0, drop
    levels = lambda *v: (C.c_double * 8)(*v)
    count = lambda *a: (lib.slnlp_selective_counts(*a, st), lib.slnlp_last_error().decode())
    #         0                 1                2  3              4  5              6  7                  8
    good_c = (p(buf["kappa"]), p(buf["rows"]), 5, levels(0.1, 1), 2, levels(0.0), 1, p(buf["counts"]), p(buf["table"]))
    assert count(*good_c)[0] == 0
    for i, value, text in [(0, None, "null pointer"), (1, None, "null pointer"), (7, None, "null pointer"), (8, None, "null pointer"),
                           (3, None, "null pointer"), (5, None, "null pointer"), (2, 0, "N=0"), (2, 1048577, "N=1048577"),
                           (4, 9, "nr=9"), (4, -1, "nr=-1"), (6, 9, "nc=9"), (3, levels(0.1, 1.5), "risks[1]=1.5"), (3, levels(-0.1), "risks[0]=-0.1"),
                           (3, levels(float("nan")), "risks[0]=nan"), (5, levels(2.0), "coverages[0]=2"), (5, levels(float("nan")), "coverages[0]=nan"),
                           (0, p(buf["kappa"]) + 4, "misaligned"), (7, p(buf["counts"]) + 4, "misaligned"),
                           (1, p(buf["rows"]) + 8, "16-byte aligned"), (8, p(buf["table"]) + 8, "32-byte aligned"),
                           (7, p(buf["kappa"]), "output counts overlaps input kappa"), (7, p(buf["rows"]) + 16, "output counts overlaps input rows"),
                           (8, p(buf["counts"]) - (p(buf["counts"]) % 32), "overlap")]:
        args = list(good_c)
        args[i] = value
        rc, msg = count(*args)
        assert rc == 1 and "selective_counts" in msg and text in msg, (i, value, rc, msg)
    args = list(good_c)
    args[3], args[4], args[5], args[6] = None, 0, None, 0                        # no levels: the arrays may be null
    assert count(*args)[0] == 0
    torch.cuda.synchronize()                                                    # no sticky error: nothing faulted
    with pytest.raises(ValueError, match="selective_rows"):
        ops.selective_rows(z.double(), y)
    with pytest.raises(ValueError, match="selective_rows"):
        ops.selective_rows(z, y.int())
    with pytest.raises(ValueError, match="selective_rows: score"):
        ops.selective_rows(z, y, score="entropy")
    with pytest.raises(ValueError, match="selective_rows: buf"):
        ops.selective_rows(z, y, ops.selective_buffers(4, "cuda"))
    with pytest.raises(ValueError, match="selective_rows: tau"):
        ops.selective_rows(z, y, tau=torch.zeros(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="selective_counts: risks"):
        ops.selective_counts(buf, risks=[1.5])
    with pytest.raises(ValueError, match="selective_buffers: N"):
        ops.selective_buffers(0, "cuda")


# ------------------------------------------------------------------------------------------------------ estimator ----
from test_calibration_gpu import make_net, raw_logp  # noqa: E402

TEMPERATURE = {"method": "temperature"}


@pytest.fixture(scope="module")
def ds():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(120, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


@pytest.fixture(scope="module")
def fitted(ds):
    """A tiny calibrated fit."""
    return make_net(ds, max_epochs=2, calibration=TEMPERATURE).partial_fit(ds)


def _raw(est, ds):
    """The float32 log-probs ``predict_proba`` downloads, before the host softmax (a wrapper's own; a fit's: uncalibrated)."""
    if "predict_nonlinearity" in est.__dict__ or hasattr(est, "module_"):
        return raw_logp(est, ds)
    est.predict_nonlinearity = "none"
    try:
        return est.predict_proba(ds)
    finally:
        del est.predict_nonlinearity


def _device_rows(z, y, beta, score):
    """The device's own kappa and rows of the downloaded log-probs ``z`` (the bytes the estimator's forward passes left)."""
    from slnlp import ops
    zd, yd = _device(z, y)
    return ops.selective_download(ops.selective_rows(zd, yd, score=score, state=ops.temperature_state(beta, "cuda") if beta != 1.0 else None),
                                  counts=False)


def _check_report(rep, z, y, beta, score, risks=(0.01, 0.05, 0.1), coverages=(0.5, 0.8, 0.9, 1.0)):
    """``risk_coverage``'s report against the restatement: kappa within the bound of the restated one, everything else as the
    restatement forms it from the DEVICE's kappa."""
    dev = _device_rows(z, y, beta, score)
    ref = sr.rows_ref(z, y, beta=beta, score=score)
    assert np.array_equal(dev["rows"], ref["rows"]) and np.abs(dev["kappa"] - ref["kappa"]).max() <= BOUND[score]
    want = sr.summary_ref(dev["kappa"], dev["rows"], risks, coverages)
    curve = sr.curve_ref(dev["kappa"], dev["rows"])
    n = want["n"]
    assert (rep["rows"], rep["errors"], rep["excluded_labels"], rep["excluded_nan"]) == (n, want["E"], 0, 0) and n == len(z)
    assert abs(rep["aurc"] - want["aurc"]) <= 2 * n * 2.0 ** -53 and rep["aurc_oracle"] == sr.aurc_oracle(n, want["E"])
    assert rep["e_aurc"] == rep["aurc"] - rep["aurc_oracle"] and rep["score"] == score
    for key in ("threshold", "accepted", "wrong", "coverage", "risk"):
        assert np.array_equal(rep["curve"][key], curve[key]), key
    assert [(e["accepted"], e["wrong"]) for e in rep["coverage_at_risk"]] == want["at_risk"]
    assert [(e["accepted"], e["wrong"]) for e in rep["risk_at_coverage"]] == want["at_coverage"]
    return dev


def test_risk_coverage_is_the_restatement_on_the_devices_kappa(ds, fitted):
    net = fitted
    beta = net.calibration_["beta"]
    assert net.temperature_ != 1.0
    z = raw_logp(net, ds)
    for score in sr.SCORES:
        rep = net.risk_coverage(ds, score=score)
        assert rep["temperature"] == net.temperature_ and np.array_equal(rep["classes"], net.classes_)
        _check_report(rep, z, ds.y, beta, score)
        print(f"{score}: accuracy {rep['accuracy']:.4f} AURC {rep['aurc']:.4f} oracle {rep['aurc_oracle']:.4f}")
    off = net.risk_coverage(ds, calibrated=False, curve=False, risks=(0.5,), coverages=())
    assert off["temperature"] == 1.0 and off["curve"] is None and off["risk_at_coverage"] == []
    on = net.risk_coverage(ds, curve=True, risks=(0.5,), coverages=())
    _check_report(on, z, ds.y, beta, "max_prob", (0.5,), ())
    assert net.risk_coverage(ds, y=ds.y, curve=False)["aurc"] == net.risk_coverage(ds, curve=False)["aurc"]
    wrong = ds.y.copy()
    wrong[3] = len(net.classes_)
    with pytest.raises(ValueError, match="risk_coverage: 1 of 120 labels lie outside the"):
        net.risk_coverage(ds, y=wrong)
    with pytest.raises(ValueError, match="fit_rejection: 1 of 120 labels lie outside the"):
        net.fit_rejection(ds, y=wrong)


def test_fit_rejection_and_predict_selective_agree_bit_for_bit(ds, fitted, tmp_path):
    from slnlp import metrics
    net = fitted
    with pytest.raises(RuntimeError, match="no rejection threshold yet"):
        net.predict_selective(ds)
    z, beta = raw_logp(net, ds), net.calibration_["beta"]
    # the fit's own labels leave next to no error on 120 rows (the Transformer's decoder sees the label) and its confidences tie in
    # a few groups, so each case judges the rows against labels of its own: the arg-max is right in the more confident half of
    # the DISTINCT confidences and wrong below.  The target then lies between the bound of that half (no error) and the bound
    # of all rows, so the threshold must fall inside the curve: conditions on the inputs, asserted
    V = len(net.classes_)
    try:
        for score, delta, calibrated, loose in [("max_prob", 0.1, True, False), ("margin", None, True, False),
                                                ("neg_entropy", 0.1, False, False), ("max_prob", 0.1, True, True)]:
            own = _device_rows(z, ds.y, beta if calibrated else 1.0, score)
            u = np.unique(own["kappa"])
            low = own["kappa"] < u[len(u) // 2]
            y_mid = np.where(low, (own["rows"][:, 0] + 1) % V, own["rows"][:, 0]).astype(np.int64)
            E, steps = int(low.sum()), max(1, math.ceil(math.log2(len(u))))
            assert len(u) >= 4 and 0 < E < 120, (score, len(u), E)
            if loose:
                target = 0.97
            elif delta is None:
                target = 0.5 * E / 120
            else:
                half, every = metrics.binomial_upper(0, 120 - E, delta / steps), metrics.binomial_upper(E, 120, delta / steps)
                assert half < every, (score, E, half, every)
                target = 0.5 * (half + every)
            assert net.fit_rejection(ds, y=y_mid, target_risk=target, delta=delta, score=score, calibrated=calibrated) is net
            r = net.rejection_
            assert set(r) == {"score", "rule", "target_risk", "delta", "threshold", "bound", "accepted", "wrong", "coverage", "risk", "n",
                              "excluded", "calibrated"}
            dev = _device_rows(z, y_mid, beta if calibrated else 1.0, score)
            rep = metrics.selective_report(dev["kappa"], dev["rows"], sr.counts_ref(dev["kappa"], dev["rows"]),
                                           sr.table_ref(dev["kappa"], dev["rows"])[0])
            want = metrics.guaranteed_threshold(rep["curve"], target, delta)
            print(f"{score} delta {delta} target {target}: {r}")
            assert want is not None and 120 - E <= r["accepted"] < (121 if loose else 120), r
            assert (r["threshold"], r["accepted"], r["wrong"], r["bound"], r["rule"]) == \
                (want["threshold"], want["accepted"], want["wrong"], want["bound"], "sgr" if delta else "empirical")
            assert r["calibrated"] is calibrated and r["n"] == 120 and r["excluded"] == 0 and r["threshold"] in dev["kappa"]
            assert net._rej_state.is_cuda and net._rej_state.cpu().numpy()[0] == r["threshold"]
            got = net.predict_selective(ds)
            assert got["accepted"].dtype == bool and got["confidence"].tobytes() == dev["kappa"].tobytes()
            assert int(got["accepted"].sum()) == r["accepted"] and np.array_equal(got["accepted"], dev["kappa"] >= r["threshold"])
            assert np.array_equal(got["labels"], net.classes_[dev["rows"][:, 0]])
            assert int((got["accepted"] & (dev["rows"][:, 0] != y_mid)).sum()) == r["wrong"] and r["target_risk"] == target
        # a save / load round trip gives the same mask
        net.save_params(str(tmp_path))
        back = make_net(ds, max_epochs=2, calibration=TEMPERATURE)
        back.load_params(str(tmp_path))
        back.classes_ = net.classes_
        assert back.rejection_ == net.rejection_ and back._rej_state.is_cuda
        assert np.array_equal(back.predict_selective(ds)["accepted"], got["accepted"])
        # nothing qualifies: 120 rows cannot show a risk of 0.1 % -- reported, not patched
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            net.fit_rejection(ds, target_risk=1e-3, delta=0.05)
        assert any(issubclass(w.category, RuntimeWarning) and "nothing is accepted" in str(w.message) for w in seen)
        r = net.rejection_
        assert r["threshold"] == np.inf and (r["accepted"], r["wrong"], r["coverage"], r["bound"]) == (0, 0, 0.0, None) and math.isnan(r["risk"])
        assert not net.predict_selective(ds)["accepted"].any()
    finally:
        net._set_rejection(None)


def test_ensemble_and_prior_shift_inherit_the_methods(ds, fitted):
    from slnlp.ensemble import VotingEnsemble
    from slnlp.prior_shift import PriorShift
    ens = VotingEnsemble([fitted, make_net(ds, seed=12, max_epochs=1).partial_fit(ds)])
    ps = PriorShift(fitted, source=np.ones(len(fitted.classes_))).set_priors(np.arange(1, len(fitted.classes_) + 1))
    for est in (ens, ps):
        with pytest.raises(RuntimeError, match="no rejection threshold yet"):
            est.predict_selective(ds)
        z = _raw(est, ds)                                                        # its own float32 log-probs, at T = 1
        for score in ("max_prob", "margin"):
            rep = est.risk_coverage(ds, score=score)
            assert rep["temperature"] == 1.0
            dev = _check_report(rep, z, ds.y, 1.0, score)
        assert est.fit_rejection(ds, target_risk=0.97, delta=None, score="margin") is est and est.rejection_["calibrated"] is False
        got = est.predict_selective(ds)
        assert got["confidence"].tobytes() == dev["kappa"].tobytes() and int(got["accepted"].sum()) == est.rejection_["accepted"] > 0
        assert np.array_equal(got["labels"], est.classes_[dev["rows"][:, 0]])
    ps.set_priors(np.ones(len(fitted.classes_)))
    assert getattr(ps, "rejection_", None) is None                               # a threshold taken under other priors does not carry over
