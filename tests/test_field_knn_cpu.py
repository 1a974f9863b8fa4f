"""CPU: the restatement of the phonology-weighted neighbour search (tests/field_knn_ref.py) -- its two forms against each other,
metric facts, F = 1 against Levenshtein -- csrc/field_edit.hpp compiled for the host against the plain program,
``ingest.field_codes`` on a hand-made vocabulary, and every check of ``PhonoKNN``, ``split_audit(field_codes=...)``,
``ops.field_*`` and the CLI key ``phono_baseline`` that raises before a GPU is needed."""
import numpy as np
import pytest

import edit_knn_ref as unit_ref
import field_knn_ref as ref

#           F  gap
METRICS = [(1, 1), (6, 6), (6, 2), (16, 16), (3, 1)]


def _table(rs, Vt, F, values=3):
    """A code table with few values per field: tokens that differ in some fields only, and distinct tokens with equal codes"""
    return rs.randint(0, values, size=(Vt, F)).astype(np.int32)


def _tokens(rs, n, Vt):
    """Mostly tokens of the table; some outside it: negative ones and 2^33 t + 7, equal in their low 32 bits"""
    t = rs.randint(0, Vt, size=n).astype(np.int64)
    kind = rs.randint(0, 8, size=n)
    t = np.where(kind == 0, -rs.randint(1, 4, size=n), t)
    return np.where(kind == 1, (rs.randint(1, 4, size=n).astype(np.int64) << 33) + 7, t)


# ---------------------------------------------------------------------------------------------------- the restatement ----
def test_hand_checked_pairs():
    codes = np.array([[0, 0, 0], [0, 0, 1], [1, 1, 1], [0, 0, 0]], dtype=np.int32)
    assert ref.sub(codes, 0, 0) == 0 and ref.sub(codes, 0, 1) == 1 and ref.sub(codes, 0, 2) == 3
    assert ref.sub(codes, 0, 3) == 0                                         # the table says which tokens are equivalent
    assert ref.sub(codes, 0, 4) == 3 and ref.sub(codes, -1, 2) == 3 and ref.sub(codes, 9, 9) == 0 and ref.sub(codes, -1, -2) == 3
    assert ref.sub(codes, 2 ** 33 + 7, 2 ** 34 + 7) == 3                     # whole int64 values
    assert ref.distance(codes, 3, [0, 2], [1, 2]) == 1
    assert ref.distance(codes, 3, [0, 2], [2]) == 3 and ref.distance(codes, 1, [0, 2], [2]) == 1
    assert ref.distance(codes, 1, [0], [2]) == 2                             # gap 1: deleting and inserting beats three fields
    assert ref.distance(codes, 3, [], [0, 1, 2]) == 9 and ref.distance(codes, 2, [0, 1], []) == 4 and ref.distance(codes, 3, [], []) == 0


@pytest.mark.parametrize("F,gap", METRICS)
def test_all_pairs_form_equals_the_plain_program(F, gap):
    """``distances`` forms each row of the two-row program for all references at once: the same integers on 480 random pairs a
    metric (tokens outside the table among them), 65535 for unusable rows, and nothing past a row's length matters"""
    rs = np.random.RandomState(10 * F + gap)
    Vt = 7
    codes = _table(rs, Vt, F)
    nq, nr, Sq, Sr = 20, 24, 10, 12
    Xq, Xr = _tokens(rs, nq * Sq, Vt).reshape(nq, Sq), _tokens(rs, nr * Sr, Vt).reshape(nr, Sr)
    Lq, Lr = rs.randint(0, Sq + 1, size=nq), rs.randint(0, Sr + 1, size=nr)
    Lq[:3], Lr[:4] = (11, -1, 0), (65, -1, 0, 12)
    D = ref.distances(Xq, Lq, Xr, Lr, codes, gap)
    assert D.dtype == np.uint16 and D.shape == (nq, nr)
    for i in range(nq):
        for j in range(nr):
            ok = 0 <= Lq[i] <= Sq and 0 <= Lr[j] <= Sr
            assert D[i, j] == (ref.distance(codes, gap, Xq[i, :Lq[i]], Xr[j, :Lr[j]]) if ok else 65535)
    Xq2, Xr2 = Xq.copy(), Xr.copy()
    for i in range(nq):
        Xq2[i, max(Lq[i], 0):] = 5
    for j in range(nr):
        Xr2[j, max(Lr[j], 0):] = 4
    assert np.array_equal(D, ref.distances(Xq2, Lq, Xr2, Lr, codes, gap))


def test_metric_facts_on_random_triples():
    rs = np.random.RandomState(0)
    for F, gap in METRICS:
        codes = _table(rs, 6, F, values=2)
        rows = [_tokens(rs, rs.randint(0, 10), 6).tolist() for _ in range(30)]
        for a in rows[:8]:
            assert ref.distance(codes, gap, a, a) == 0
        for _ in range(120):
            a, b, c = (rows[i] for i in rs.randint(0, len(rows), size=3))
            ab, bc, ac = ref.distance(codes, gap, a, b), ref.distance(codes, gap, b, c), ref.distance(codes, gap, a, c)
            assert ab == ref.distance(codes, gap, b, a)
            if gap == F:
                assert ac <= ab + bc
            assert abs(len(a) - len(b)) * gap <= ab <= F * max(len(a), len(b))


def test_one_field_is_levenshtein():
    rs = np.random.RandomState(3)
    codes = np.arange(9, dtype=np.int32)[:, None]
    for _ in range(200):
        a, b = rs.randint(0, 9, size=rs.randint(0, 14)), rs.randint(0, 9, size=rs.randint(0, 14))
        assert ref.distance(codes, 1, a, b) == unit_ref.levenshtein(a, b)
    X, L = rs.randint(0, 9, size=(12, 9)), rs.randint(0, 10, size=12)
    D = ref.distances(X, L, X, L, codes, 1)
    U = unit_ref.distances(X, L, X, L)
    assert np.array_equal(D.astype(np.int64), U.astype(np.int64))


def test_selection_bound_and_vote_unit():
    dist = np.array([[7, 3, 3, 65535, 3, 0], [65535] * 6], dtype=np.uint16)
    Lq, Lr = np.array([4, 70]), np.array([4, 4, 4, -1, 4, 4])
    res = ref.knn_rows(dist, Lq, Lr, 8, 8, 3, F=3, radius=3, exclude=np.array([5, -1]))
    assert res["nbr"][0].tolist() == [[3, 1], [3, 2], [3, 4]] and res["rows"][0].tolist() == [3, 3, 3, 0]
    assert res["nbr"][1].tolist() == [[-1, -1]] * 3 and res["rows"][1].tolist() == [0, 0, -1, 1] and res["head"][:2].tolist() == [1, 1]
    prior = np.array([0.5, 0.5])
    one = {"rows": np.array([[1, 0, 6, 0]], dtype=np.int32), "nbr": np.array([[[6, 0]]], dtype=np.int32)}
    z, bad = ref.knn_logp(one, [4], [2], [1], prior, F=3, tau=1.0, normalize=True, lam=1.0)
    w = np.exp(-6.0 / (3 * 4))                                               # tau is in frames: d / F per frame
    assert bad == 0 and np.allclose(np.exp(z[0].astype(np.float64)), np.array([0.5, w + 0.5]) / (w + 1.0), rtol=1e-6)
    z1, _ = ref.knn_logp(one, [4], [2], [1], prior, F=1)
    u1, _ = unit_ref.knn_logp(one, [4], [2], [1], prior)
    assert z1.tobytes() == u1.tobytes()


def test_the_header_equals_the_plain_program(tmp_path):
    """csrc/field_edit.hpp -- the cost function and the column step the kernel runs per reference token -- compiled for the host and
    held to the two-row program on 20000 random pairs (tests/field_edit_check.cpp)"""
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "field_edit_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-o", exe, os.path.join(here, "field_edit_check.cpp")], check=True)
    done = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert done.returncode == 0 and done.stdout.strip().endswith("20000 pairs, 0 bad"), done.stdout


# ------------------------------------------------------------------------------------------------------- field_codes ----
class _Vocab:
    def __init__(self, words):
        self.itos = list(words)
        self.stoi = {w: i for i, w in enumerate(self.itos)}

    def __len__(self):
        return len(self.itos)


def test_field_codes_on_a_hand_made_vocabulary():
    from slnlp import ingest
    fields = ["orientation_dh", "movement_dh", "handshape_dh"]
    v = _Vocab(["<unk>", "<pad>", "ldf-ru-5", "ldf-ru-b", "rub-ru-5", "odd-token", "ldf--5"])
    got = ingest.field_codes(v, fields, "as_words")
    assert got.dtype == np.int32 and got.shape == (7, 3)
    assert got.tolist() == [[-1] * 3, [-2] * 3, [0, 0, 0], [0, 0, 1], [1, 0, 0], [-6] * 3, [0, 1, 0]]
    assert (got[2] != got[3]).sum() == 1                                     # two tokens one field apart: cost 1
    assert ref.sub(got, 2, 3) == 1 and ref.sub(got, 2, 4) == 1 and ref.sub(got, 3, 4) == 2 and ref.sub(got, 2, 5) == 3 and ref.sub(got, 0, 1) == 3
    assert np.array_equal(ingest.field_codes(v, fields, "as_words_norm"), got)
    wide = _Vocab(["<unk>", "<pad>", f"{'left':<20}-{'up':<20}-{'5':<20}", f"{'left':<20}-{'down':<20}-{'5':<20}", "x-y"])
    assert ingest.field_codes(wide, fields, "all_values").tolist() == [[-1] * 3, [-2] * 3, [0, 0, 0], [0, 1, 0], [-5] * 3]
    sep = _Vocab(["<unk>", "<pad>", "['ldf', 'ru', '5']", "['ldf', 'ru', 'b']", "['ldf', 'ru']", "not a list"])
    assert ingest.field_codes(sep, fields, "as_sep_feat").tolist() == [[-1] * 3, [-2] * 3, [0, 0, 0], [0, 0, 1], [-5] * 3, [-6] * 3]
    with pytest.raises(ValueError, match="Unknown composition strategy"):
        ingest.field_codes(v, fields, "as_letters")
    with pytest.raises(ValueError, match="field_codes: no fields"):
        ingest.field_codes(v, [], "as_words")


# ----------------------------------------------------------------------------------- checks that need no GPU ----
def _dataset(n=6, S=5, lengths=None, vocab=None):
    from slnlp.data import TokenDataset
    rs = np.random.RandomState(2)
    return TokenDataset(rs.randint(2, 9, size=(n, S)), rs.randint(1, S + 1, size=n) if lengths is None else lengths, rs.randint(0, 3, size=n), vocab)


def test_exported_and_the_unit_surface_is_unchanged():
    import slnlp
    from slnlp import cli, edit_knn
    assert slnlp.PhonoKNN is edit_knn.PhonoKNN and issubclass(slnlp.PhonoKNN, slnlp.EditKNN) and "PhonoKNN" in slnlp.__all__
    assert slnlp.EditKNN().get_params() == dict(k=5, weights="distance", tau=1.0, normalize=True, smoothing=1.0, device=None)
    assert cli.baseline_options({}) == {"k": 5, "weights": "distance", "tau": 1.0, "normalize": True, "smoothing": 1.0, "radius": 2, "top": 50}


def test_estimator_options_and_refusals_before_the_gpu():
    import slnlp
    from sklearn.base import clone
    codes = np.arange(18, dtype=np.int32).reshape(9, 2)
    knn = slnlp.PhonoKNN(codes)
    assert list(knn.get_params()) == ["device", "field_codes", "gap", "k", "normalize", "smoothing", "tau", "weights"]
    assert knn.get_params()["gap"] is None and knn.get_params()["field_codes"] is codes and clone(knn).get_params()["k"] == 5
    assert not knn.initialized_ and knn.calibration_ is None
    for bad, text in ((np.zeros(4, dtype=np.int32), "2-D integer array"), (np.zeros((4, 17), dtype=np.int32), "2-D integer array"),
                      (np.zeros((0, 3), dtype=np.int32), "2-D integer array"), (np.zeros((4, 2)), "2-D integer array"),
                      (np.full((2, 2), 2 ** 31, dtype=np.int64), "outside int32")):
        with pytest.raises(ValueError, match=f"PhonoKNN: field_codes.*{text}"):
            slnlp.PhonoKNN(bad)
    for gap in (0, 3, True, 1.0):
        with pytest.raises(ValueError, match="PhonoKNN: gap="):
            slnlp.PhonoKNN(codes, gap=gap)
    with pytest.raises(ValueError, match="EditKNN: k=0"):
        slnlp.PhonoKNN(codes, k=0)
    with pytest.raises(ValueError, match="expected a cuda device"):
        slnlp.PhonoKNN(codes, device="cpu")
    with pytest.raises(RuntimeError, match="not initialized"):
        knn.predict_proba(_dataset())
    vocab = _Vocab([f"t{i}" for i in range(10)])                            # ten tokens, nine rows in the table
    with pytest.raises(ValueError, match="PhonoKNN.fit: field_codes has 9 rows, the dataset's source vocabulary 10 tokens"):
        knn.fit(_dataset(vocab=vocab))
    with pytest.raises(ValueError, match=r"EditKNN.fit: 1 of 6 rows have a length outside 0..5"):
        knn.fit(_dataset(lengths=[1, 6, 2, 3, 5, 0]))
    knn.gap = 5                                                             # set_params goes past __init__: fit checks again
    with pytest.raises(ValueError, match="PhonoKNN: gap=5"):
        knn.fit(_dataset())


def test_split_audit_refusals_before_the_gpu():
    import slnlp
    ds = _dataset()
    codes = np.zeros((9, 3), dtype=np.int32)
    with pytest.raises(ValueError, match="split_audit: radius=193"):
        slnlp.split_audit(ds, ds, radius=193, field_codes=codes)
    with pytest.raises(ValueError, match="split_audit: radius=65"):
        slnlp.split_audit(ds, ds, radius=65)                                # the unit-cost bound stays
    with pytest.raises(ValueError, match="split_audit: gap=4"):
        slnlp.split_audit(ds, ds, field_codes=codes, gap=4)
    with pytest.raises(ValueError, match="split_audit: gap=1 without field_codes"):
        slnlp.split_audit(ds, ds, gap=1)
    with pytest.raises(ValueError, match="split_audit: field_codes must be a 2-D integer array"):
        slnlp.split_audit(ds, ds, field_codes=np.zeros(3))
    with pytest.raises(ValueError, match="split_audit: field_codes has 9 rows, the source vocabulary of train 10 tokens"):
        slnlp.split_audit(_dataset(vocab=_Vocab(range(10))), ds, field_codes=codes)
    with pytest.raises(TypeError):
        slnlp.split_audit(ds, ds, 2, 50, None, None, codes)                  # keyword-only
    with pytest.raises(ValueError, match="expected a cuda device"):
        slnlp.split_audit(ds, ds, field_codes=codes, device="cpu")


def test_reports_take_the_metric_bound():
    from slnlp import metrics
    rows = np.array([[1, 1, 70, 0], [1, 0, 192, 0], [0, 0, -1, 1]], dtype=np.int32)
    nbr = np.array([[[70, 1]], [[192, 0]], [[-1, -1]]], dtype=np.int32)
    yq, yr = np.array([0, 1, 1]), np.array([1, 1])
    res = metrics.split_audit_report(rows, nbr, yq, yr, 100, 10, max_distance=192)
    assert res["nearest_hist"].shape == (194,) and res["nearest_hist"][[70, 192, 193]].tolist() == [1, 1, 1] and res["near_duplicates"] == 1
    assert metrics.knn_report(rows, nbr, yq, yr, max_distance=192)["nearest_hist"].shape == (194,)
    assert metrics.knn_report(rows, nbr, yq, yr)["nearest_hist"].shape == (66,)           # the default is the unit metric's
    with pytest.raises(ValueError, match="split_audit_report: radius=193"):
        metrics.split_audit_report(rows, nbr, yq, yr, 193, 10, max_distance=192)
    with pytest.raises(ValueError, match="split_audit_report: max_distance=1025"):
        metrics.split_audit_report(rows, nbr, yq, yr, 2, 10, max_distance=1025)
    with pytest.raises(ValueError, match="knn_report: max_distance=0"):
        metrics.knn_report(rows, nbr, yq, yr, max_distance=0)


def test_ops_argument_checks():
    import torch
    from slnlp import ops
    X, L = torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    codes = torch.zeros(5, 3, dtype=torch.int32)
    for k in (0, 65, 2.0):
        with pytest.raises(ValueError, match="field_knn_rows: k="):
            ops.field_knn_rows(X, L, X, L, codes, k)
    buf = ops.edit_knn_buffers(3, 2, "cpu")
    prior = torch.full((3,), 1 / 3, dtype=torch.float64)
    for F in (0, 17, True):
        with pytest.raises(ValueError, match="field_knn_logp: F="):
            ops.field_knn_logp(buf, L, L, L, prior, F)
    with pytest.raises(ValueError, match="field_knn_logp: weights='rank'"):
        ops.field_knn_logp(buf, L, L, L, prior, 3, weights="rank")
    with pytest.raises(ValueError, match="field_knn_logp: tau=0"):
        ops.field_knn_logp(buf, L, L, L, prior, 3, tau=0)
    with pytest.raises(ValueError, match="field_knn_logp: buf must be edit_knn_buffers"):
        ops.field_knn_logp({"shape": (3,)}, L, L, L, prior, 3)
    for bad in (torch.zeros(5, 3, dtype=torch.int64), torch.zeros(5, 17, dtype=torch.int32), torch.zeros(5, dtype=torch.int32),
                torch.zeros(3, 5, dtype=torch.int32).t()):
        with pytest.raises(ValueError, match="_field_table: codes must be a contiguous int32"):
            ops._field_table("_field_table", bad, None, torch.device("cpu"))
    assert ops._field_table("t", codes, None, torch.device("cpu")) == (5, 3, 3) and ops._field_table("t", codes, 2, torch.device("cpu")) == (5, 3, 2)
    for gap in (0, 4, 1.5):
        with pytest.raises(ValueError, match="t: gap="):
            ops._field_table("t", codes, gap, torch.device("cpu"))


def test_cli_key():
    from slnlp import cli
    assert cli.phono_baseline_options(None) is None and "phono_baseline" in cli.DICT_ARGS and "baseline" in cli.DICT_ARGS
    assert cli.phono_baseline_options({}) == {"k": 5, "weights": "distance", "tau": 1.0, "normalize": True, "smoothing": 1.0, "gap": None,
                                              "radius": None, "top": 50}
    assert cli.phono_baseline_options({"gap": 2, "radius": 0})["gap"] == 2
    for bad, text in ((5, "expected a dict"), ({"neighbours": 3}, "unknown keys"), ({"k": 0}, "k=0"), ({"weights": "rank"}, "weights='rank'"),
                      ({"tau": 0}, "tau=0"), ({"smoothing": "1"}, "smoothing='1'"), ({"normalize": 1}, "normalize=1"), ({"gap": 0}, "gap=0"),
                      ({"gap": 17}, "gap=17"), ({"gap": True}, "gap=True"), ({"radius": 1025}, "radius=1025"), ({"radius": -1}, "radius=-1"),
                      ({"top": -1}, "top=-1")):
        with pytest.raises(ValueError, match=f"phono_baseline.*{text}"):
            cli.phono_baseline_options(bad)
    ds = _dataset()
    with pytest.raises(ValueError, match="phono_baseline: needs dataset_args.fields"):
        cli.phono_field_codes(ds, {"fields": ["a", "b"]})                    # no vocabulary that names the tokens
    with pytest.raises(ValueError, match="phono_baseline: needs dataset_args.fields"):
        cli.phono_field_codes(_dataset(vocab=_Vocab(["<unk>", "<pad>", "a-b"])), {})
    with pytest.raises(ValueError, match="phono_baseline: 17 fields"):
        cli.phono_field_codes(_dataset(vocab=_Vocab(["<unk>", "<pad>", "a-b"])), {"fields": [f"f{i}" for i in range(17)]})
    got = cli.phono_field_codes(_dataset(vocab=_Vocab(["<unk>", "<pad>", "a-b", "a-c"])), {"fields": ["x", "y"]})
    assert got.tolist() == [[-1, -1], [-2, -2], [0, 0], [0, 1]]
    opts = cli.phono_baseline_options({"gap": 3})
    with pytest.raises(ValueError, match=r"phono_baseline: gap=3, expected null or an integer in 1..2"):
        cli.save_phono_baseline(None, ds, ds, opts, None, None, ["accuracy"], "cuda", ".", field_codes=got)
    opts = cli.phono_baseline_options({"radius": 129})
    with pytest.raises(ValueError, match=r"phono_baseline: radius=129, expected null or an integer in 0..128"):
        cli.save_phono_baseline(None, ds, ds, opts, None, None, ["accuracy"], "cuda", ".", field_codes=got)
    assert "phono_baseline:" in cli.__doc__ and "test_phono_split_audit.json" in cli.__doc__ and "baseline_vs_phono" in cli.__doc__
