"""CPU: the multi-word bit-vector recurrence (csrc/edit_myers_multi.hpp) held to the plain two-row program under the host
compiler's address and undefined-behaviour sanitizers, the restatement of the long-row search (tests/edit_long_ref.py) against
``levenshtein``, and every ``max_len`` check of ``EditKNN``, ``PhonoKNN``, ``split_audit`` and the CLI key that raises before a GPU is
needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import edit_long_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sign-language-nlp_amd", "csrc")


def _dataset(n=6, S=8, length=4, seed=0):
    from slnlp.data import TokenDataset
    rs = np.random.RandomState(seed)
    return TokenDataset(rs.randint(2, 9, size=(n, S)).astype(np.int64), np.full(n, length), np.arange(n) % 3)


# ---------------------------------------------------------------------------------------------------- the recurrence ----
def test_the_multi_word_recurrence_equals_the_plain_program_under_sanitizers(tmp_path):
    """tests/edit_myers_multi_check.cpp: a stand-alone program (its own main) built with -fsanitize=address,undefined by the host
    compiler -- 3000 random pairs, alphabets of 1 to 5 tokens that differ only above bit 32, half the lengths at the word edges up
    to 512, a third of the equal-length pairs identical, every W the kernel instantiates.  Nothing is loaded into this process."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "edit_myers_multi_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe,
                    os.path.join(HERE, "edit_myers_multi_check.cpp")], check=True)
    done = subprocess.run([exe, "3000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0 and done.stdout.strip().startswith("pairs=3000") and done.stdout.strip().endswith("bad=0"), done.stdout + done.stderr
    assert "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, done.stderr


# ---------------------------------------------------------------------------------------------------- the restatement ----
def test_restatement_equals_levenshtein_on_long_pairs():
    rs = np.random.RandomState(2)
    S = 140
    Lq, Lr = np.array([0, 1, 64, 65, 128, 129, 130, 131, -1]), np.array([130, 0, 63, 129, 131, 7])
    Xq, Xr = rs.randint(0, 3, size=(len(Lq), S)), rs.randint(0, 3, size=(len(Lr), S + 2))
    D = ref.distances(Xq, Lq, Xr, Lr, 130)
    assert D.dtype == np.uint16 and D.shape == (len(Lq), len(Lr))
    for i in range(len(Lq)):
        for j in range(len(Lr)):
            ok = 0 <= Lq[i] <= 130 and 0 <= Lr[j] <= 130
            assert D[i, j] == (ref.levenshtein(Xq[i, :Lq[i]], Xr[j, :Lr[j]]) if ok else 65535)
    assert (D[7] == 65535).all() and (D[:, 4] == 65535).all()           # 131 > max_len although it fits the row
    narrow = ref.distances(Xq[:, :100], Lq, Xr, Lr, 130)                # the row's width binds before max_len does
    assert (narrow[4:8] == 65535).all() and np.array_equal(narrow[:4], D[:4])
    Xq2 = Xq.copy()
    for i in range(len(Lq)):
        Xq2[i, max(Lq[i], 0):] = 99
    assert np.array_equal(D, ref.distances(Xq2, Lq, Xr, Lr, 130))      # nothing past a row's length matters


def test_restatement_selection_head_and_vote():
    import edit_knn_ref as short
    dist = np.array([[300, 100, 100, 65535, 100, 0], [65535] * 6, [256, 256, 256, 65535, 256, 256]], dtype=np.uint16)
    Lq, Lr = np.array([400, 600, 300]), np.array([400, 400, 400, -1, 400, 400])
    res = ref.knn_rows(dist, Lq, Lr, 512, 512, 3, 512, radius=100, exclude=np.array([5, -1, 7]))
    assert res["nbr"][0].tolist() == [[100, 1], [100, 2], [100, 4]] and res["rows"][0].tolist() == [3, 3, 100, 0]
    assert res["nbr"][1].tolist() == [[-1, -1]] * 3 and res["rows"][1].tolist() == [0, 0, -1, 1]
    assert res["nbr"][2].tolist() == [[256, 0], [256, 1], [256, 2]] and res["rows"][2].tolist() == [3, 0, 256, 2]
    assert res["head"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    assert ref.knn_rows(dist, Lq, Lr, 512, 512, 3, 399)["head"].tolist()[:2] == [2, 6]        # max_len binds: 400 > 399, and the -1
    prior = ref.prior_of([0, 1, 1], 2)
    z, bad = ref.knn_logp(res, Lq, Lr, [0, 1, 1, 0, 0, 1], prior, 512, tau=0.5)
    want, _ = short.knn_logp(res, Lq, Lr, [0, 1, 1, 0, 0, 1], prior, tau=0.5)
    assert bad == 0 and np.array_equal(z, want, equal_nan=True) and np.isnan(z[1]).all() and np.isfinite(z[[0, 2]]).all()
    with pytest.raises(AssertionError):
        ref.knn_logp(res, Lq, Lr, [0, 1, 1, 0, 0, 1], prior, 255)      # a neighbour beyond the bound is not this search's


# ------------------------------------------------------------------------------------------------------- the options ----
def test_editknn_max_len_checks_and_params():
    import slnlp
    from sklearn.base import clone
    assert slnlp.EditKNN().get_params() == {"k": 5, "weights": "distance", "tau": 1.0, "normalize": True, "smoothing": 1.0, "device": None}
    assert slnlp.EditKNN().max_len is None
    knn = slnlp.EditKNN(k=3, max_len=128)
    assert knn.get_params()["max_len"] == 128 and clone(knn).get_params() == knn.get_params() and clone(knn).max_len == 128
    assert "max_len" not in clone(slnlp.EditKNN()).get_params()
    assert slnlp.EditKNN().set_params(max_len=200, k=2).get_params()["max_len"] == 200
    assert "max_len" not in knn.set_params(max_len=None).get_params()
    for bad in (64, 0, 513, -1, 128.0, True, "128"):
        with pytest.raises(ValueError, match="EditKNN: max_len="):
            slnlp.EditKNN(max_len=bad)
        late = slnlp.EditKNN()
        late.set_params(max_len=bad)                         # set_params goes past __init__: fit checks again
        with pytest.raises(ValueError, match="EditKNN: max_len="):
            late.fit(_dataset())


def test_fit_checks_rows_against_max_len_before_the_gpu():
    import slnlp
    from slnlp.data import TokenDataset
    long = TokenDataset(np.zeros((3, 140), dtype=np.int64), [64, 130, 131], [0, 1, 0])
    with pytest.raises(ValueError, match=r"2 of 3 rows have a length outside 0..64 \(first: row 1, length 130\); rows longer than 64 frames are refused"):
        slnlp.EditKNN().fit(long)                            # today's message
    with pytest.raises(ValueError, match=r"1 of 3 rows have a length outside 0..130 \(first: row 2, length 131\); rows longer than 130 frames are refused"):
        slnlp.EditKNN(max_len=130).fit(long)
    narrow = TokenDataset(np.zeros((2, 100), dtype=np.int64), [100, 101], [0, 1])
    with pytest.raises(ValueError, match=r"1 of 2 rows have a length outside 0..100 "):
        slnlp.EditKNN(max_len=512).fit(narrow)               # the row's width binds first
    with pytest.raises(ValueError, match="EditKNN.fit: 1 of 3 labels lie outside"):
        slnlp.EditKNN(max_len=131).fit(TokenDataset(np.zeros((3, 140), dtype=np.int64), [64, 130, 131], [0, 1, -1]))


def test_phonoknn_refuses_max_len():
    import slnlp
    codes = np.arange(20).reshape(10, 2)
    with pytest.raises(TypeError, match="max_len"):
        slnlp.PhonoKNN(codes, max_len=128)
    knn = slnlp.PhonoKNN(codes)
    assert "max_len" not in knn.get_params()
    knn.max_len = 128
    with pytest.raises(ValueError, match="PhonoKNN.fit: max_len=128: the phonology-weighted search is limited to 64 frames"):
        knn.fit(_dataset())
    with pytest.raises(ValueError, match="limited to 64 frames"):
        slnlp.PhonoKNN(codes).set_params(max_len=200).fit(_dataset())


def test_split_audit_max_len_checks():
    import slnlp
    ds = _dataset()
    for bad in (64, 513, 0, 2.5, True):
        with pytest.raises(ValueError, match="split_audit: max_len="):
            slnlp.split_audit(ds, ds, max_len=bad)
    with pytest.raises(ValueError, match="split_audit: radius=129"):
        slnlp.split_audit(ds, ds, radius=129, max_len=128)
    with pytest.raises(ValueError, match="split_audit: radius=65"):
        slnlp.split_audit(ds, ds, radius=65)                 # unchanged without max_len
    with pytest.raises(ValueError, match="split_audit: max_len=128 with field_codes: the phonology-weighted search is limited to 64 frames"):
        slnlp.split_audit(ds, ds, field_codes=np.arange(20).reshape(10, 2), max_len=128)
    with pytest.raises(ValueError, match="expected a cuda device"):
        slnlp.split_audit(ds, ds, radius=128, max_len=128, device="cpu")      # every check above passed


def test_cli_key_max_len():
    from slnlp import cli
    assert cli.baseline_options({}) == {"k": 5, "weights": "distance", "tau": 1.0, "normalize": True, "smoothing": 1.0, "radius": 2, "top": 50}
    got = cli.baseline_options({"max_len": 128, "radius": 100})
    assert got == {"k": 5, "weights": "distance", "tau": 1.0, "normalize": True, "smoothing": 1.0, "radius": 100, "top": 50, "max_len": 128}
    for bad, text in (({"max_len": 64}, "max_len=64"), ({"max_len": 513}, "max_len=513"), ({"max_len": True}, "max_len=True"),
                      ({"max_len": None}, "max_len=None"), ({"max_len": 128, "radius": 129}, r"radius=129, expected an integer in 0\.\.128"),
                      ({"radius": 65}, r"radius=65, expected an integer in 0\.\.64")):
        with pytest.raises(ValueError, match=f"baseline.*{text}"):
            cli.baseline_options(bad)
    with pytest.raises(ValueError, match="phono_baseline: unknown keys .'max_len'."):
        cli.phono_baseline_options({"max_len": 128})
    assert "max_len: 128" in cli.__doc__ and "stays at 64 frames" in cli.__doc__


def test_ops_int_checks_and_two_bytes_a_pair():
    import torch
    from slnlp import ops
    from slnlp.edit_knn import SCRATCH_PAIRS, query_chunks
    X, L = torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError):
        ops.edit_long_distances(X, L, X, L)                  # max_len is a required keyword
    with pytest.raises(TypeError):
        ops.edit_long_knn_rows(X, L, X, L, 2)
    with pytest.raises(ValueError, match="edit_long_distances: max_len=128.0"):
        ops.edit_long_distances(X, L, X, L, max_len=128.0)
    for k in (0, 65, 2.0):
        with pytest.raises(ValueError, match="edit_long_knn_rows: k="):
            ops.edit_long_knn_rows(X, L, X, L, k, max_len=128)
    buf = ops.edit_knn_buffers(3, 2, "cpu")
    prior = torch.full((3,), 1 / 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="edit_long_knn_logp: weights='rank'"):
        ops.edit_long_knn_logp(buf, L, L, L, prior, max_len=128, weights="rank")
    with pytest.raises(TypeError):
        ops.edit_long_knn_logp(buf, L, L, L, prior)
    # the long search keeps two bytes a pair: chunked at half the pairs, the scratch stays at 256 MiB
    chunks = query_chunks(40000, 10000, SCRATCH_PAIRS // 2)
    assert all(2 * (b - a) * 10000 <= SCRATCH_PAIRS for a, b in chunks) and len(chunks) == 3 and chunks[-1][1] == 40000
    assert chunks[0][0] == 0 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    assert query_chunks(16384, 16384, SCRATCH_PAIRS // 2) == [(0, 8192), (8192, 16384)] and query_chunks(16384, 16384) == [(0, 16384)]
