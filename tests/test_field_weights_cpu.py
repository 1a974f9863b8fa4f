"""CPU: per-field integer weights of the phonology-weighted edit distance -- the restatement (tests/field_weight_ref.py) against
hand-computed distances and against its own plain program, csrc/field_edit.hpp's weighted column step compiled for the host (plain
and with -fsanitize=address,undefined: a stand-alone binary, nothing is loaded into python), every refusal of
``slnlp_field_distances_w`` / ``slnlp_field_knn_rows_w`` / ``slnlp_loo_objective`` by its text (they are raised before a device
is touched), the option checks of ``PhonoKNN(field_weights=)``, ``split_audit``, ``fit_field_weights`` and the CLI sub-key, and
the search logic over a fake evaluator."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import field_knn_ref as unit_ref
import field_weight_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------------------------------- the restatement ----
def test_hand_checked_distances():
    codes = np.array([[0, 0, 0], [0, 0, 1], [1, 1, 1], [0, 1, 0]], dtype=np.int32)
    w = (2, 0, 1)                                                            # W = 3
    assert ref.sub(codes, w, 0, 0) == 0 and ref.sub(codes, w, 0, 1) == 1 and ref.sub(codes, w, 0, 2) == 3
    assert ref.sub(codes, w, 0, 3) == 0                                      # a weight-0 field makes two distinct tokens equivalent
    assert ref.sub(codes, w, 1, 3) == 1 and ref.sub(codes, w, 2, 3) == 3
    assert ref.sub(codes, (0, 5, 0), 0, 3) == 5 and ref.sub(codes, (0, 5, 0), 0, 1) == 0
    assert ref.sub(codes, w, 0, 4) == 3 and ref.sub(codes, w, -1, 2) == 3 and ref.sub(codes, w, 9, 9) == 0          # outside: W
    assert ref.sub(codes, (4, 0, 8), 0, 4) == 12 and ref.sub(codes, (4, 0, 8), 2 ** 33 + 7, 2 ** 34 + 7) == 12       # W, never F = 3
    assert ref.distance(codes, w, 3, [0, 2], [3, 2]) == 0                    # equivalent rows: an exact duplicate
    assert ref.distance(codes, w, 3, [0, 2], [1, 2]) == 1 and ref.distance(codes, w, 3, [0, 2], [2]) == 3
    assert ref.distance(codes, w, 1, [0], [2]) == 2                          # gap 1: delete and insert beat the substitution of 3
    assert ref.distance(codes, w, 2, [], [0, 1, 2]) == 6 and ref.distance(codes, w, 3, [], []) == 0


@pytest.mark.parametrize("w,gap", [((1, 1, 1, 1), 4), ((4, 0, 2, 0), 6), ((4, 0, 2, 0), 1), ((0, 0, 0, 16), 16), ((3, 1, 0, 2), 2)])
def test_all_pairs_form_equals_the_plain_program(w, gap):
    rs = np.random.RandomState(sum(w) + gap)
    Vt, F = 7, 4
    codes = rs.randint(0, 3, size=(Vt, F)).astype(np.int32)
    tok = lambda n: np.where(rs.rand(n) < 0.2, -rs.randint(1, 4, size=n), rs.randint(0, Vt + 1, size=n)).astype(np.int64)
    nq, nr, Sq, Sr = 10, 12, 8, 9
    Xq, Xr = tok(nq * Sq).reshape(nq, Sq), tok(nr * Sr).reshape(nr, Sr)
    Lq, Lr = rs.randint(0, Sq + 1, size=nq), rs.randint(0, Sr + 1, size=nr)
    Lq[:2], Lr[:3] = (9, -1), (65, -1, 0)
    D = ref.distances(Xq, Lq, Xr, Lr, codes, w, gap)
    for i in range(nq):
        for j in range(nr):
            ok = 0 <= Lq[i] <= Sq and 0 <= Lr[j] <= Sr
            assert D[i, j] == (ref.distance(codes, w, gap, Xq[i, :Lq[i]], Xr[j, :Lr[j]]) if ok else 65535)
    if set(w) == {1}:                                                        # all ones: the unweighted restatement
        assert np.array_equal(D, unit_ref.distances(Xq, Lq, Xr, Lr, codes, gap))


def test_objective_restatement():
    z = np.log(np.array([[0.5, 0.5, 0.0], [0.2, 0.3, 0.5], [0.1, 0.8, 0.1], [np.nan, 0.5, 0.5], [0.3, 0.3, 0.4]], dtype=np.float32) + 1e-9)
    y = np.array([1, 2, 0, 1, 7])
    right, total, nans, bad = ref.loo_objective(z, y)
    assert (right, nans, bad) == (1, 1, 1)                                   # row 0 ties: the lower index 0 wins, the label is 1
    assert total == pytest.approx(-(np.float64(z[0, 1]) + np.float64(z[1, 2]) + np.float64(z[2, 0])))
    v = np.random.RandomState(0).rand(1000)
    assert ref.tree_sum(v) == pytest.approx(v.sum(), rel=1e-13) and ref.tree_sum(v[:1]) == v[0] and ref.tree_sum([]) == 0.0


# --------------------------------------------------------------------------------------------------------- the header ----
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_weighted_column_step_equals_the_plain_program(tmp_path, sanitize):
    """csrc/field_edit.hpp's weighted count and column step, compiled for the host into a stand-alone program with its own main
    and held to the two-row program on 20000 random pairs (tests/field_weight_check.cpp)"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "field_weight_check")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([cxx, "-O1", "-std=c++17", *flags, "-o", exe, os.path.join(HERE, "field_weight_check.cpp")], check=True)
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and done.stdout.strip().endswith("20000 pairs, 0 bad"), done.stdout


# ---------------------------------------------------------------------------------------------------------- refusals ----
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    return _lib.load()


def test_library_refusals_by_their_text(lib):
    """Every refusal of the weighted entry points and of ``slnlp_loo_objective`` comes before anything is launched: the pointers
    are addresses inside a host array that nothing reads"""
    mem = (C.c_char * 16384)()
    base = (C.addressof(mem) + 63) // 64 * 64
    Xq, Lq, Xr, Lr, codes, scratch, head, rows, nbr, dist = (base + 1024 * i for i in range(10))
    ok_w = (C.c_int32 * 3)(2, 0, 1)
    wp = lambda *v: (C.c_int32 * len(v))(*v)

    def rows_w(F=3, w=ok_w, gap=1, radius=0, k=2, scratch_bytes=64, **over):
        a = dict(Xq=Xq, Lq=Lq, Xr=Xr, Lr=Lr, codes=codes, scratch=scratch, head=head, rows=rows, nbr=nbr)
        a.update(over)
        return lib.slnlp_field_knn_rows_w(a["Xq"], 4, a["Lq"], 3, a["Xr"], 4, a["Lr"], 2, a["codes"], 40, F, w, gap, None, k, radius, a["scratch"],
                                          scratch_bytes, a["head"], a["rows"], a["nbr"], None)

    def dist_w(F=3, w=ok_w, gap=1, **over):
        a = dict(codes=codes, dist=dist)
        a.update(over)
        return lib.slnlp_field_distances_w(Xq, 4, Lq, 3, Xr, 4, Lr, 2, a["codes"], 40, F, w, gap, a["dist"], None)

    def refused(rc, text):
        msg = lib.slnlp_last_error().decode()
        assert rc == 1 and text in msg, (rc, msg)
    for call, what in ((rows_w, "field_knn_rows_w"), (dist_w, "field_distances_w")):
        refused(call(w=None), f"{what}: null pointer (fweights: a host array of F weights)")
        refused(call(w=wp(2, 17, 1)), f"{what}: fweights[1]=17 outside 0..16")
        refused(call(w=wp(2, -1, 1)), f"{what}: fweights[1]=-1 outside 0..16")
        refused(call(w=wp(0, 0, 0)), f"{what}: the weights sum to W=0 outside 1..16")
        refused(call(w=wp(8, 8, 1)), f"{what}: the weights sum to W=17 outside 1..16")
        refused(call(gap=0), f"{what}: gap=0 outside 1..W=3")
        refused(call(gap=4), f"{what}: gap=4 outside 1..W=3")                # F = 3 too: the gap is held to W
        refused(call(F=4, w=wp(1, 0, 0, 0), gap=2), f"{what}: gap=2 outside 1..W=1")
        refused(call(F=0), f"{what}: F=0 outside 1..16")
        refused(call(F=17), f"{what}: F=17 outside 1..16")
        refused(call(codes=None), f"{what}: null pointer (codes)")
        refused(call(codes=codes + 1), f"{what}: misaligned pointer (codes: 4 bytes)")
    refused(rows_w(radius=64 * 3 + 1), "field_knn_rows_w: radius=193 outside 0..64 W=192")
    refused(rows_w(radius=-1), "field_knn_rows_w: radius=-1 outside 0..64 W=192")
    refused(rows_w(F=6, w=wp(1, 0, 0, 0, 0, 0), radius=65), "field_knn_rows_w: radius=65 outside 0..64 W=64")       # W, not F = 6
    refused(rows_w(k=0), "field_knn_rows_w: k=0 outside 1..64")
    refused(rows_w(Xq=None), "field_knn_rows_w: null pointer (query rows)")
    refused(rows_w(scratch=None), "field_knn_rows_w: null pointer (scratch, head, rows or nbr)")
    refused(rows_w(scratch_bytes=3), "field_knn_rows_w: scratch of 3 bytes is too small")
    refused(rows_w(scratch=scratch + 1), "field_knn_rows_w: scratch is not 2-byte aligned")
    refused(rows_w(rows=rows + 2), "field_knn_rows_w: misaligned pointer (head, exclude: 8 bytes; rows, nbr: 4 bytes)")
    refused(rows_w(codes=scratch), "field_knn_rows_w: output scratch overlaps input codes")
    refused(rows_w(nbr=rows), "field_knn_rows_w: outputs rows and nbr overlap")
    refused(dist_w(dist=None), "field_distances_w: null pointer (dist)")
    refused(dist_w(dist=dist + 1), "field_distances_w: misaligned pointer (dist: 2 bytes)")
    refused(dist_w(dist=codes), "field_distances_w: output dist overlaps input codes")
    # the unweighted entries keep their words: F, where the weighted ones say W
    rc = lib.slnlp_field_knn_rows(Xq, 4, Lq, 3, Xr, 4, Lr, 2, codes, 40, 3, 4, None, 2, 0, scratch, 64, head, rows, nbr, None)
    refused(rc, "field_knn_rows: gap=4 outside 1..F=3")
    rc = lib.slnlp_field_knn_rows(Xq, 4, Lq, 3, Xr, 4, Lr, 2, codes, 40, 3, 1, None, 2, 193, scratch, 64, head, rows, nbr, None)
    refused(rc, "field_knn_rows: radius=193 outside 0..64 F=192")

    def objective(logp=Xq, y=Lq, table=head, N=5, V=3, ld=3, slots=4, slot=0):
        return lib.slnlp_loo_objective(logp, ld, y, N, V, table, slots, slot, None)
    refused(objective(logp=None), "loo_objective: null pointer")
    refused(objective(N=0), "loo_objective: N=0 outside 1..")
    refused(objective(V=0), "loo_objective: V=0 outside 1..")
    refused(objective(ld=2), "loo_objective: ld=2 is less than V=3")
    refused(objective(slots=0), "loo_objective: C=0 slots outside 1..65536")
    refused(objective(slot=4), "loo_objective: slot=4 outside 0..C-1=3")
    refused(objective(slot=-1), "loo_objective: slot=-1 outside 0..C-1=3")
    refused(objective(table=head + 4), "loo_objective: misaligned pointer")
    refused(objective(table=Xq), "loo_objective: output table overlaps input logp")


# ------------------------------------------------------------------------------------------- options before the GPU ----
def _dataset(n=6, S=5, lengths=None, vocab=None):
    from slnlp.data import TokenDataset
    rs = np.random.RandomState(2)
    return TokenDataset(rs.randint(2, 9, size=(n, S)), rs.randint(1, S + 1, size=n) if lengths is None else lengths, rs.randint(0, 3, size=n), vocab)


def test_estimator_option_checks():
    import slnlp
    from sklearn.base import clone
    codes = np.arange(27, dtype=np.int32).reshape(9, 3)
    assert "fit_field_weights" in slnlp.__all__ and callable(slnlp.fit_field_weights)
    plain = slnlp.PhonoKNN(codes)
    assert "field_weights" not in plain.get_params() and plain.field_weights is None          # the unweighted list is what it was
    knn = slnlp.PhonoKNN(codes, field_weights=(2, 0, 1), gap=3)
    assert knn.get_params()["field_weights"] == (2, 0, 1) and clone(knn).get_params()["field_weights"] == (2, 0, 1)
    assert clone(knn).set_params(field_weights=None).get_params().get("field_weights") is None
    assert plain.set_params(field_weights=[1, 1, 2]).field_weights == [1, 1, 2]
    for bad in ((1, 1), (1, 1, 1, 1), (1, -1, 1), (17, 0, 0), (1.0, 1, 1), (True, 1, 1), 3, "abc"):
        with pytest.raises(ValueError, match="PhonoKNN: field_weights="):
            slnlp.PhonoKNN(codes, field_weights=bad)
    with pytest.raises(ValueError, match=r"PhonoKNN: field_weights=\(0, 0, 0\) sum to W=0"):
        slnlp.PhonoKNN(codes, field_weights=(0, 0, 0))
    with pytest.raises(ValueError, match=r"PhonoKNN: field_weights=\(8, 8, 1\) sum to W=17"):
        slnlp.PhonoKNN(codes, field_weights=(8, 8, 1))
    slnlp.PhonoKNN(codes, field_weights=(4, 0, 8), gap=12)                   # the gap goes up to W = 12, past F = 3
    for gap in (0, 4, True):
        with pytest.raises(ValueError, match="PhonoKNN: gap="):
            slnlp.PhonoKNN(codes, field_weights=(2, 0, 1), gap=gap)
    with pytest.raises(ValueError, match="PhonoKNN: gap=4"):
        slnlp.PhonoKNN(codes, gap=4)                                         # without weights the bound stays F
    knn.field_weights = (1, 0, 0)                                            # past __init__: fit checks again (gap 3 > W = 1)
    with pytest.raises(ValueError, match="PhonoKNN: gap=3"):
        knn.fit(_dataset())
    knn.field_weights = (1, 0)
    with pytest.raises(ValueError, match="PhonoKNN: field_weights="):
        knn.fit(_dataset())


def test_split_audit_and_ops_option_checks():
    import slnlp
    import torch
    from slnlp import ops
    ds = _dataset()
    codes = np.zeros((9, 3), dtype=np.int32)
    with pytest.raises(ValueError, match=r"split_audit: field_weights=\(1, 1, 1\) without field_codes"):
        slnlp.split_audit(ds, ds, field_weights=(1, 1, 1))
    with pytest.raises(ValueError, match="split_audit: field_weights="):
        slnlp.split_audit(ds, ds, field_codes=codes, field_weights=(1, 1))
    with pytest.raises(ValueError, match="split_audit: radius=129"):
        slnlp.split_audit(ds, ds, radius=129, field_codes=codes, field_weights=(2, 0, 0))       # 64 W = 128, not 64 F = 192
    with pytest.raises(ValueError, match="split_audit: gap=3"):
        slnlp.split_audit(ds, ds, field_codes=codes, field_weights=(2, 0, 0), gap=3)
    with pytest.raises(ValueError, match="expected a cuda device"):
        slnlp.split_audit(ds, ds, radius=128, field_codes=codes, field_weights=(2, 0, 0), gap=2, device="cpu")
    fw, W, gap = ops._field_weights("t", [4, 0, 2], 3, None)
    assert list(fw) == [4, 0, 2] and (W, gap) == (6, 6) and ops._field_weights("t", np.array([4, 0, 2]), 3, 5)[2] == 5
    with pytest.raises(ValueError, match="t: gap=7"):
        ops._field_weights("t", [4, 0, 2], 3, 7)
    with pytest.raises(ValueError, match="loo_objective_table: slots=0"):
        ops.loo_objective_table(0, "cpu")
    assert tuple(ops.loo_objective_table(3, "cpu").shape) == (3, 4)
    with pytest.raises(ValueError, match="loo_objective: logp must be a float32"):
        ops.loo_objective(torch.zeros(3, 2), torch.zeros(3, dtype=torch.int64), ops.loo_objective_table(1, "cpu"), 0)


def test_fit_field_weights_option_checks():
    import slnlp
    ds = _dataset()
    codes = np.zeros((9, 3), dtype=np.int32)
    for kw, text in ((dict(levels=()), "levels="), (dict(levels=(0, 17)), "levels="), (dict(levels=(1, 1)), "levels="), (dict(levels=(1.0,)), "levels="),
                     (dict(sweeps=0), "sweeps=0"), (dict(scoring="f1"), "scoring='f1'"), (dict(start=(1, 1)), "start="), (dict(start=(0, 0, 0)), "start="),
                     (dict(start=(9, 9, 0)), "start="), (dict(gap=0), "gap=0"), (dict(gap=4), "gap=4 exceeds the start's W=3"),
                     (dict(neighbours=3), "unknown options"), (dict(k=0), "k=0")):
        with pytest.raises(ValueError, match=f"(fit_field_weights|EditKNN|PhonoKNN).*{text}"):
            slnlp.fit_field_weights(ds, codes, **kw)
    with pytest.raises(ValueError, match="fit_field_weights: field_codes must be a 2-D integer array"):
        slnlp.fit_field_weights(ds, np.zeros(3))
    doc = slnlp.fit_field_weights.__doc__
    assert "leave-one-out on the TRAIN split" in doc and "split_audit(train, train)" in doc and "held-out rows" in doc


def test_cli_sub_key():
    from slnlp import cli
    base = {"k": 5, "weights": "distance", "tau": 1.0, "normalize": True, "smoothing": 1.0, "gap": None, "radius": None, "top": 50}
    assert cli.phono_baseline_options({}) == base and cli.phono_baseline_options({"fit_weights": None}) == base
    got = cli.phono_baseline_options({"k": 3, "fit_weights": {}})
    assert got["fit_weights"] == {"levels": [0, 1, 2, 4], "sweeps": 2, "scoring": "neg_log_loss"} and got["k"] == 3
    assert cli.phono_baseline_options({"fit_weights": {"levels": [0, 1, 3], "scoring": "accuracy"}})["fit_weights"]["levels"] == [0, 1, 3]
    for bad, text in ((5, "=5, expected null or a dict"), ({"level": [1]}, "unknown keys"), ({"levels": []}, "levels="), ({"levels": [0, 17]}, "levels="),
                      ({"levels": [1, 1]}, "levels="), ({"levels": "012"}, "levels="), ({"sweeps": 0}, "sweeps=0"), ({"sweeps": True}, "sweeps=True"),
                      ({"scoring": "f1"}, "scoring='f1'")):
        with pytest.raises(ValueError, match=f"phono_baseline: fit_weights.*{text}"):
            cli.phono_baseline_options({"fit_weights": bad})
    with pytest.raises(ValueError, match=r"phono_baseline: unknown keys \['neighbours'\] \(known: \('k', 'weights', 'tau', 'normalize', 'smoothing', 'gap', "
                                         r"'radius', 'top'\)\)"):
        cli.phono_baseline_options({"neighbours": 3})                        # the same words as before
    assert "fit_weights" in cli.__doc__ and "train_phono_weights.json" in cli.__doc__ and "phono_vs_weighted" in cli.__doc__


# ---------------------------------------------------------------------------------------------------- the search logic ----
def test_search_logic_with_a_fake_evaluator():
    from slnlp.field_weights import coordinate_search
    calls = []

    def table(fn):
        def evaluate(field, cands):
            calls.append((field, list(cands)))
            return [fn(c) for c in cands]
        return evaluate
    # the sum falls with w0 and rises with w1; w2 changes nothing: ties go to the smaller W
    res = coordinate_search(3, table(lambda w: (sum(w), 10.0 - w[0] + w[1])))
    assert res["weights_unreduced"] == (4, 0, 0) and res["weights"] == (1, 0, 0) and res["converged"] and res["sweeps_run"] == 2
    assert res["start_objective"] == -10.0 and res["objective"] == -6.0 and res["evaluations"] == len(res["trace"]) == 1 + sum(len(c) for _, c in calls[1:])
    assert calls[0] == (None, [(1, 1, 1)]) and calls[1] == (0, [(0, 1, 1), (1, 1, 1), (2, 1, 1), (4, 1, 1)])
    assert calls[4] == (0, [(1, 0, 0), (2, 0, 0), (4, 0, 0)])               # (0, 0, 0): W = 0 is skipped, never evaluated
    assert res["steps"][:3] == [(4, 1, 1), (4, 0, 1), (4, 0, 0)] and [t["field"] for t in res["trace"][:6]] == [None, 0, 0, 0, 0, 1]
    # candidates past W = 16 are skipped; the restatement walks the same path
    calls.clear()
    fn = lambda w: (0, -float(sum(w)))
    res = coordinate_search(2, table(fn), levels=(1, 8, 16), sweeps=3)
    assert all(1 <= sum(c) <= 16 for _, cs in calls for c in cs) and res["weights_unreduced"] == (8, 8) and res["weights"] == (1, 1)
    want = ref.coordinate_search(2, fn, levels=(1, 8, 16), sweeps=3)
    assert want["unreduced"] == (8, 8) and want["steps"] == res["steps"] and want["converged"] == res["converged"]
    assert coordinate_search(2, table(fn), levels=(1, 8, 16), sweeps=3, reduce=False)["weights"] == (8, 8)
    # accuracy ranks by the count; equal counts: the smaller W, then the lexicographically smaller vector
    res = coordinate_search(2, table(lambda w: (5, 0.0)), levels=(2, 1), scoring="accuracy")
    assert res["weights_unreduced"] == (1, 1) and res["converged"] and res["sweeps_run"] == 1 and res["objective"] == 5
    res = coordinate_search(2, table(lambda w: (7 if sum(w) == 3 else 5, 0.0)), levels=(1, 2), scoring="accuracy", sweeps=1)
    assert res["weights_unreduced"] == (2, 1) and not res["converged"]       # (2, 1) is met first and is not beaten by (1, 2) later
    # a start whose value is no level stays a candidate, so a step never loses ground
    res = coordinate_search(2, table(lambda w: (0, abs(w[0] - 3) + abs(w[1] - 3))), levels=(0, 1), start=(3, 3))
    assert res["weights_unreduced"] == (3, 3) and res["weights"] == (1, 1) and res["converged"]
    for kw in (dict(levels=()), dict(sweeps=0), dict(scoring="auc"), dict(start=(1,))):
        with pytest.raises(ValueError, match="coordinate_search: "):
            coordinate_search(2, table(fn), **kw)
    # the library's search and the restatement's agree on a rugged made-up objective, both scorings
    rs = np.random.RandomState(4)
    noise = rs.rand(5, 5, 5)
    rugged = lambda w: (int(10 * noise[w[0] % 5, w[1] % 5, w[2] % 5]), float(noise[w[2] % 5, w[0] % 5, w[1] % 5]))
    for scoring in ("neg_log_loss", "accuracy"):
        got = coordinate_search(3, table(rugged), scoring=scoring, sweeps=4)
        want = ref.coordinate_search(3, rugged, scoring=scoring, sweeps=4)
        assert got["steps"] == want["steps"] and got["weights"] == want["weights"] and got["sweeps_run"] == want["sweeps_run"]
        assert [(t["field"], t["weights"], t["right"], t["sum"]) for t in got["trace"]] == want["trace"]
