"""CPU: the host side of the voting ensembles -- the numpy restatement the GPU tests lean on (tests/ensemble_ref.py) against a
direct computation (a plain fp64 softmax per member, the weighted mean, -sum p log p), the margin that lets the GPU tests compare
the arg-max on every row, the edge rules, ``metrics.uncertainty_summary``, the option checks of the estimator and the CLI key,
and the C ABI's declarations and argument checks (the library loads without a GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ensemble_ref import (FAMILIES, SHAPES, case_betas, case_weights, direct_ref, ensemble_ref, make_members, normalised, out_bound,
                          spacing32, top_gap, uncertainty_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROSS = [(shape, family, betas_on, weights_on) for shape in SHAPES for family in FAMILIES for betas_on in (False, True)
         for weights_on in (False, True)]


@pytest.fixture(scope="module")
def cases():
    """Every case of the issue, both modes: (shape, family, betas_on, weights_on, mode) -> (members, betas, weights, out, rows)."""
    got = {}
    for (N, V, K), family, betas_on, weights_on in CROSS:
        members, _ = make_members(N, V, K, *family)
        betas, weights = case_betas(K, betas_on), case_weights(K, weights_on)
        for mode in ("soft", "log"):
            got[(N, V, K), family, betas_on, weights_on, mode] = (members, betas, weights, *ensemble_ref(members, betas, weights, mode))
    return got


def test_the_generator_is_the_issues():
    from test_calibration_cpu import make_logp
    members, y = make_members(5, 3, 2, 2.0, 0.6, 3)
    base, y0 = make_logp(5, 3, 2.0, 0.6, 3)
    assert np.array_equal(y, y0) and len(members) == 2
    z = base.astype(np.float64) + 0.5 * 2.0 * np.random.RandomState(3001).randn(5, 3)
    z -= z.max(axis=1, keepdims=True)
    assert np.array_equal(members[1], (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32))
    assert not np.array_equal(members[0], members[1]) and members[0].dtype == np.float32
    assert np.array_equal(normalised([1.0, 2.0, 3.0], 3), np.array([1.0, 2.0, 3.0]) / 6.0) and np.array_equal(normalised(None, 4), np.full(4, 0.25))


def test_restatement_against_the_direct_computation(cases):
    worst = 0.0
    for (shape, family, betas_on, weights_on, mode), (members, betas, weights, out, rows) in cases.items():
        tag = (shape, family, betas_on, weights_on, mode)
        K = shape[2]
        w = normalised(weights, K)
        pbar, h_total, h_mean = direct_ref(members, betas, weights)
        assert np.isfinite(out).all() and np.isfinite(rows).all(), tag
        if mode == "soft":                                   # the mean of the probabilities
            want = pbar
        else:                                                # their weighted geometric mean, renormalised
            logs = sum(w[k] * np.log(direct_ref([members[k]], [betas[k]])[0]) for k in range(K))
            want = np.exp(logs - logs.max(axis=1, keepdims=True))
            want /= want.sum(axis=1, keepdims=True)
        assert np.abs(np.exp(out) - want).max() <= 1e-12, tag
        assert np.abs(np.exp(out).sum(axis=1) - 1.0).max() <= 1e-12, tag
        # the decomposition, whatever the mode: the mixture's entropy, the members' expected entropy, their difference
        d = max(np.abs(rows[:, 0] - h_total).max(), np.abs(rows[:, 1] - h_mean).max(), np.abs(rows[:, 2] - (h_total - h_mean)).max())
        worst = max(worst, d)
        assert d <= 1e-11, (tag, d)                          # (the direct difference cancels: that is the looser side)
        assert rows[:, 2].min() >= -1e-12 and rows[:, 2].max() <= -(w * np.log(w)).sum() + 1e-12, tag
        assert ((rows[:, 3] >= 0) & (rows[:, 3] <= K) & (rows[:, 3] == np.round(rows[:, 3]))).all(), tag
        if K == 1:
            assert not rows[:, 3].any() and np.abs(rows[:, 2]).max() <= 1e-15 and np.abs(rows[:, 0] - rows[:, 1]).max() <= 1e-12, tag
    print(f"{len(cases)} cases; max |restatement - direct| over the three entropies: {worst:.3g}")


def test_every_row_has_a_clear_winner(cases):
    """What lets the GPU tests compare the arg-max and n_disagree on EVERY row: the restatement's gap between the two largest
    ``out`` values exceeds 1e-5 everywhere, while the float32 spacing of the winner is below 1e-6 and the device may be off by
    ``out_bound`` on either value -- no device rounding can move a first maximum."""
    smallest, where = np.inf, None
    for tag, (_, _, _, out, _) in cases.items():
        if tag[0][1] == 1:
            continue
        gap = top_gap(out)
        two = np.sort(out, axis=1)[:, -2:]
        assert spacing32(two[:, 1]).max() < 1e-6 and (gap > 2.0 * out_bound(two).sum(axis=1)).all(), tag
        if gap.min() < smallest:
            smallest, where = gap.min(), tag
        assert gap.min() > 1e-5, (tag, gap.min())
    print(f"smallest gap between the top two out values: {smallest:.3g} at {where}")
    assert where[0] == (300, 202, 4) and where[1][2] == 3 and where[3] and where[4] == "log" and abs(smallest - 4.04e-5) < 1e-7


def test_edge_rules():
    # V = 1: out 0 and no entropy, whatever the members hold
    one = [np.array([[0.0], [-3.0], [2.5], [0.0]], dtype=np.float32), np.zeros((4, 1), dtype=np.float32)]
    for mode in ("soft", "log"):
        out, rows = ensemble_ref(one, [0.16, None], [1.0, 2.0], mode)
        assert np.abs(out).max() <= 1e-15 and np.abs(rows).max() <= 1e-15
    members, _ = make_members(9, 7, 3, 2.0, 0.6, 5)
    clean = {mode: ensemble_ref(members, mode=mode) for mode in ("soft", "log")}
    # a NaN entry in one member's row: that row is NaN with code -2, every other row is untouched
    nan = [m.copy() for m in members]
    nan[1][4, 2] = np.nan
    for mode in ("soft", "log"):
        out, rows = ensemble_ref(nan, mode=mode)
        assert np.isnan(out[4]).all() and np.array_equal(rows[4], [np.nan, np.nan, np.nan, -2.0], equal_nan=True)
        keep = np.arange(9) != 4
        assert np.array_equal(out[keep], clean[mode][0][keep]) and np.array_equal(rows[keep], clean[mode][1][keep])
    # a -inf column shared by all members (never a member's maximum): probability 0 in both modes, every number still finite elsewhere
    shared = [m.copy() for m in members]
    col = int(np.argmin(sum(m[6] for m in members)))
    for m in shared:
        m[6, col] = -np.inf
    for mode in ("soft", "log"):
        out, rows = ensemble_ref(shared, mode=mode)
        assert out[6, col] == -np.inf and np.isfinite(np.delete(out[6], col)).all() and np.isfinite(rows).all()
        assert abs(np.exp(out[6]).sum() - 1.0) <= 1e-12
    # a -inf column in a single member: the mixture keeps the others' mass, the product of experts has none there
    single = [m.copy() for m in members]
    single[2][6, col] = -np.inf
    soft, rows = ensemble_ref(single, mode="soft")
    assert np.isfinite(soft).all() and np.isfinite(rows).all() and rows[6, 2] > 0.0
    want = (np.exp(clean["soft"][0][6, col]) * 3.0 - np.exp(members[2][6, col].astype(np.float64))) / 3.0
    assert abs(np.exp(soft[6, col]) - want) <= 1e-6          # (the member's other columns were not renormalised: nearly the rest)
    log, rows = ensemble_ref(single, mode="log")
    assert log[6, col] == -np.inf and np.isfinite(np.delete(log[6], col)).all() and np.isfinite(rows).all()
    # log mode, every class impossible for some member: the NaN row; the soft vote of the same row is an ordinary one
    split = [np.array([[0.0, -np.inf]], dtype=np.float32), np.array([[-np.inf, 0.0]], dtype=np.float32)]
    out, rows = ensemble_ref(split, mode="log")
    assert np.isnan(out).all() and np.array_equal(rows[0], [np.nan, np.nan, np.nan, -2.0], equal_nan=True)
    out, rows = ensemble_ref(split, mode="soft")
    assert np.allclose(out, np.log(0.5), atol=1e-15) and abs(rows[0, 0] - np.log(2.0)) <= 1e-15 and rows[0, 1] == 0.0
    assert abs(rows[0, 2] - np.log(2.0)) <= 1e-15 and rows[0, 3] == 1.0      # the largest MI two members can have; one of them is outvoted
    # a row whose maximum is not finite
    for bad in (np.inf, -np.inf):
        rowless = [np.full((1, 3), bad, dtype=np.float32), np.zeros((1, 3), dtype=np.float32)]
        out, rows = ensemble_ref(rowless)
        assert np.isnan(out).all() and rows[0, 3] == -2.0
    # the bound's two parts
    assert out_bound(np.array([-1.0]))[0] == 0.5 * 2.0 ** -23 + 1e-9 and out_bound(np.array([-300.0]))[0] == 0.5 * 2.0 ** -15 + 3e-7


def test_uncertainty_summary():
    from slnlp import metrics
    members, _ = make_members(33, 7, 3, 2.0, 0.6, 2)
    members[0][5, 1] = np.nan
    _, rows = ensemble_ref(members, weights=[1.0, 2.0, 3.0])
    got = metrics.uncertainty_summary(rows)
    assert got == uncertainty_ref(rows) and got["rows"] == 32 and got["nan_rows"] == 1
    assert set(got) == {"total_entropy", "expected_entropy", "mutual_information", "disagreement_rate", "mean_disagreement", "rows", "nan_rows"}
    ok = rows[:, 3] >= 0
    assert got["total_entropy"] == rows[ok, 0].sum() / 32 and got["disagreement_rate"] == (rows[ok, 3] > 0).sum() / 32
    assert abs(got["total_entropy"] - got["expected_entropy"] - got["mutual_information"]) <= 1e-12
    assert 0.0 < got["disagreement_rate"] <= 1.0 and got["disagreement_rate"] <= got["mean_disagreement"] <= 3.0
    none = metrics.uncertainty_summary(np.array([[np.nan, np.nan, np.nan, -2.0]]))
    assert none["rows"] == 0 and none["nan_rows"] == 1 and np.isnan(none["mutual_information"]) and np.isnan(none["disagreement_rate"])
    with pytest.raises(ValueError, match="uncertainty_summary: rows has shape"):
        metrics.uncertainty_summary(np.zeros((3, 3)))


def test_estimator_surface_without_a_gpu():
    import slnlp
    from slnlp.ensemble import VotingEnsemble
    from slnlp.net import NeuralNetClassifier
    assert slnlp.VotingEnsemble is VotingEnsemble
    # the consumers of one fit's log-probs are the estimator's own functions, not copies
    for name in ("predict_proba", "predict", "score", "predict_topk", "reliability", "error_analysis", "score_interval", "compare"):
        assert getattr(VotingEnsemble, name) is getattr(NeuralNetClassifier, name), name

    def fitted(n_classes, device="cuda:0"):
        net = NeuralNetClassifier(module="model.Transformer", device=device)
        net.initialized_, net.classes_ = True, np.arange(n_classes)
        return net
    a, b = fitted(6), fitted(6)
    with pytest.raises(RuntimeError, match="initialized"):
        VotingEnsemble([a, NeuralNetClassifier(module="model.Transformer")])
    for members in ([], None, a, [a, "b"], [a] * 33):
        with pytest.raises(ValueError, match="VotingEnsemble: members must be a list of 1..32"):
            VotingEnsemble(members)
    with pytest.raises(ValueError, match=r"different classes_ \(7 and 6 classes\)"):
        VotingEnsemble([a, fitted(7)])
    with pytest.raises(ValueError, match="member 1 is on cuda:1, member 0 on cuda:0"):
        VotingEnsemble([a, fitted(6, "cuda:1")])
    for voting in ("hard", None, 0):
        with pytest.raises(ValueError, match="VotingEnsemble: voting="):
            VotingEnsemble([a, b], voting=voting)
    for weights in ([1.0], [1.0, 0.0], [1.0, -1.0], [1.0, float("inf")], [1.0, float("nan")], 2.0):
        with pytest.raises(ValueError, match="VotingEnsemble: weights must be 2 finite numbers above 0"):
            VotingEnsemble([a, b], weights=weights)
    ens = VotingEnsemble([a, b], voting="log", weights=[1, 3], calibrated=False)
    assert ens.calibration_ is None and ens.temperature_ == 1.0 and ens.initialized_ and np.array_equal(ens.classes_, np.arange(6))
    assert (ens.voting, ens.weights, ens.calibrated, ens.members) == ("log", [1.0, 3.0], False, [a, b])
    # the bound methods check their options before anything runs, as on a fit
    with pytest.raises(ValueError, match="score_interval: replicates="):
        ens.score_interval(None, replicates=0)
    with pytest.raises(ValueError, match="predict_topk: k=7"):
        ens.predict_topk(None, k=7)
    with pytest.raises(ValueError, match=r"compare: the two fits have different classes_ \(6 and 7 classes\)"):
        ens.compare(fitted(7), None)
    with pytest.raises(ValueError, match=r"compare: the two fits have different classes_ \(7 and 6 classes\)"):
        fitted(7).compare(ens, None)


def test_cli_key_is_validated():
    from slnlp import cli
    assert cli.ensemble_options(None) is None
    assert cli.ensemble_options({}) == {"members": 5, "voting": "soft"}
    assert cli.ensemble_options({"members": 3, "voting": "log"}) == {"members": 3, "voting": "log"}
    assert "ensemble" in cli.DICT_ARGS
    for bad, text in (([], "expected a dict"), ({"member": 3}, "unknown keys"), ({"members": 1}, "members=1"), ({"members": 33}, "members=33"),
                      ({"members": 2.0}, "members=2.0"), ({"members": True}, "members=True"), ({"voting": "hard"}, "voting='hard'")):
        with pytest.raises(ValueError, match=text):
            cli.ensemble_options(bad)


def test_the_entry_point_is_declared_and_bound():
    from slnlp import _lib, ops
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    text = src[src.index("ensembles of log-probs"):src.index("slnlp_ensemble_rows(")]
    for said in ("log1p(rest_k + (n_at_max_k - 1))", "m_c + log(sum_k w_k exp(l_kc - m_c))", "sum_k w_k sum_c p_kc (l_kc - mix_c)",
                 "summed directly", "as stored", "(NaN, NaN, NaN, -2)", "out may alias NO input", "by value"):
        assert said in text, f"the header states the rule so that a caller can restate it: {said!r}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                  # the way tests/test_abi.py reads the header
    assert "slnlp_ensemble_rows" in set(re.findall(r"\b(slnlp_[a-z0-9_]+)\s*\(", src))
    assert len(_lib.SIGNATURES["slnlp_ensemble_rows"][1]) == 12
    for macro, value, mirror in (("SLNLP_ENSEMBLE_MAX_MEMBERS", 32, _lib.ENSEMBLE_MAX_MEMBERS), ("SLNLP_VOTE_SOFT", 0, _lib.VOTING["soft"]),
                                 ("SLNLP_VOTE_LOG", 1, _lib.VOTING["log"])):
        (found,), = [re.findall(rf"#define {macro}\s+(\d+)", src)]
        assert int(found) == value == mirror, macro
    for fn in ("ensemble_rows", "ensemble_download"):
        assert callable(getattr(ops, fn)), fn
    hip = re.sub(r"//.*", "", open(os.path.join(ROOT, "sign-language-nlp_amd", "csrc", "ensemble.hip")).read())
    assert "SLNLP_ZKERNEL" in hip and hip.count("zlaunch(") == 1 and "SLNLP_CHECK_ARG" in hip
    assert "hipMalloc" not in hip and "hipMemcpy" not in hip and "atomic" not in hip and "__shared__" not in hip
    assert "wave_sum_d" in hip and "wave_best" in hip
    assert "csrc/ensemble.hip" in open(os.path.join(ROOT, "sign-language-nlp_amd", "Makefile")).read()


def test_the_library_exports_it_and_checks_its_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    lib = _lib.load()
    assert lib.slnlp_abi_version() == 1
    # every check comes before the launch, so a machine without a GPU can ask for the codes and messages (the device pointers
    # are never read: they are numbers here; the arrays of them are host memory, as the entry point takes them)
    N, V, K = 5, 3, 3
    members, betas, out, rows = [1 << 20, 2 << 20, 3 << 20], [4 << 20, None, 5 << 20], 6 << 20, 7 << 20

    def call(**kw):
        a = dict(members=members, ld=[3, 4, 3], betas=betas, weights=[1.0, 2.0, 3.0], K=K, N=N, V=V, mode=0, out=out, ld_out=3, rows=rows)
        a.update(kw)
        arr = lambda t, v: None if v is None else (t * len(v))(*v)
        rc = lib.slnlp_ensemble_rows(arr(C.c_void_p, a["members"]), arr(C.c_int64, a["ld"]), arr(C.c_void_p, a["betas"]),
                                     arr(C.c_double, a["weights"]), a["K"], a["N"], a["V"], a["mode"], a["out"], a["ld_out"], a["rows"], None)
        return rc, lib.slnlp_last_error().decode()
    big = 2 ** 31
    for kw, text in (({"members": None}, "null pointer"), ({"ld": None}, "null pointer"), ({"out": None}, "null pointer"),
                     ({"members": [1 << 20, None, 3 << 20]}, "member 1 is a null pointer"), ({"K": 0}, "K=0 outside 1..32"),
                     ({"K": 33}, "K=33 outside 1..32"), ({"N": 0}, "N=0 outside"), ({"N": big}, f"N={big} outside"), ({"V": 0}, "V=0 outside"),
                     ({"V": big}, f"V={big} outside"), ({"mode": 2}, "mode=2"), ({"mode": -1}, "mode=-1"),
                     ({"ld": [3, 2, 3]}, "ld[1]=2 is less than V=3"), ({"ld_out": 2}, "ld_out=2 is less than V=3"),
                     ({"weights": [1.0, 0.0, 1.0]}, "weights[1]=0 is not a finite number above 0"), ({"weights": [1.0, 1.0, -2.0]}, "weights[2]=-2"),
                     ({"weights": [float("inf"), 1.0, 1.0]}, "weights[0]=inf"), ({"weights": [1.0, float("nan"), 1.0]}, "weights[1]=nan"),
                     ({"members": [(1 << 20) + 2, 2 << 20, 3 << 20]}, "member 0 is not 4-byte aligned"), ({"out": out + 2}, "out is not 4-byte aligned"),
                     ({"betas": [(4 << 20) + 4, None, None]}, "beta of member 0 is not 8-byte aligned"),
                     ({"rows": rows + 16}, "rows is not 32-byte aligned"), ({"out": (2 << 20) + 16}, "out overlaps member 1"),
                     ({"out": (2 << 20) + 4 * 18}, "out overlaps member 1"),       # its last float: 4 rows of 4 floats, then 3
                     ({"out": 1 << 20}, "out overlaps member 0"), ({"rows": (3 << 20) + 32}, "rows overlaps member 2"),
                     ({"out": (5 << 20) - 4}, "out overlaps the beta of member 2"), ({"rows": 4 << 20}, "rows overlaps the beta of member 0"),
                     ({"rows": out + 32}, "out and rows overlap")):
        rc, msg = call(**kw)
        assert rc == 1 and "ensemble_rows" in msg and text in msg, (kw, rc, msg)
