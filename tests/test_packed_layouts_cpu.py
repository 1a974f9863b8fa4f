"""The packed judging buffers of slnlp.ops against tests/golden/packed_layouts.json, which tools/record_layouts.py wrote from the
commit before the buffers moved onto slnlp/_packed.py: no layout moves by a byte and every download cuts the same bytes."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorded(golden_dir):
    spec = importlib.util.spec_from_file_location("record_layouts", os.path.join(ROOT, "tools", "record_layouts.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(golden_dir, "packed_layouts.json")) as f:
        want = json.load(f)
    return json.loads(json.dumps(tool.record())), want      # (through JSON: tuples and integer keys as the file holds them)


@pytest.mark.parametrize("section", ["layouts", "downloads"])
def test_the_tree_matches_the_recording(recorded, section):
    got, want = (r[section] for r in recorded)
    assert sorted(got) == sorted(want) and len(want) >= (75 if section == "layouts" else 150)
    for name in want:
        assert got[name] == want[name], f"{section} {name}"


def test_the_grid_holds_the_shapes_where_a_padding_rule_flips(recorded):
    names = "\n".join(recorded[1]["layouts"])
    for said in ("_N1_", "_N2_", "_N5_", "_N8_", "_N2049_", "_V1", "_V3", "_V32", "_V33", "_V202", "_kNone_", "_k1_", "_k3_", "_M1", "_M20",
                 "_M64", "conformal_N5_V32_sets0", "conformal_N5_V32_sets1", "ranking_N5_V32_rows0", "bootstrap_N5_V32_counts0",
                 "bootstrap_B7_V2_Q0", "_bins1", "_bins15", "attribution_N5_V32_M3_", "attribution_N5_V32_M4_"):
        assert said in names, said
    flat = {n: v["tensors"]["flat"]["shape"][0] for n, v in recorded[1]["layouts"].items() if "flat" in v["tensors"]}
    assert flat["selective_N2049_V202"] - flat["selective_N5_V32"] == 4 * (2049 - 5) + 1 + 1        # a second chunk word, and one pad entry
    assert flat["conformal_N8_V33_sets1"] - flat["conformal_N8_V33_sets0"] == 8                     # 8 rows of two set words
    assert flat["conformal_N5_V32_sets1"] - flat["conformal_N5_V32_sets0"] == 3                     # 5 rows of one: they end inside an int64


def test_one_copy_for_slices_of_one_allocation_and_one_each_otherwise(monkeypatch):
    import torch
    from slnlp import _packed, ops
    copies, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append((t.numel(), t.dtype)) or real(t, *a, **k))

    def counted(fn, *args):
        del copies[:]
        fn(*args)
        return list(copies)
    N, V, k = 5, 3, 3
    score, topk, boot = ops.score_buffers(N, V, "cpu"), ops.topk_buffers(N, k, "cpu"), ops.bootstrap_buffers(7, 2, 3, True, "cpu")
    assert counted(ops.score_download, score) == [(3 * N + 3 * V + 1, torch.int32)]
    assert counted(ops.topk_download, topk) == [(3 * N * k, torch.int32)]
    assert counted(ops.bootstrap_download, boot) == [(7 * 12 + (7 * 7 + 1) // 2, torch.float64)]       # 49 int32 counts end inside a word
    assert counted(ops.bootstrap_download, ops.bootstrap_buffers(7, 2, 3, False, "cpu")) == [(7 * 12, torch.float64)]
    for fn, out in ((ops.score_download, score), (ops.topk_download, topk), (ops.bootstrap_download, boot)):
        each = sorted((t.numel(), str(t.dtype)) for t in out)
        assert sorted((n, str(d)) for n, d in counted(fn, tuple(t.clone() for t in out))) == each           # separate allocations
        assert sorted((n, str(d)) for n, d in counted(fn, out[::-1])) == each                                # one allocation, out of order
    ea = ops.error_analysis_buffers(N, V, k, 4, "cpu")      # its score pieces: counts lie BEFORE pred; its top-k lists: idx before prob
    assert len(counted(ops.score_download, ea["score"])) == 4 and len(counted(ops.topk_download, ea["topk"])) == 2
    flat = torch.arange(12, dtype=torch.int32)
    assert counted(_packed.download, (flat[0:3], flat[4:6]), torch.int32) == [(3, torch.int32), (2, torch.int32)]      # a hole of a whole unit
    assert counted(_packed.download, (flat[0:3], flat[3:6]), torch.int64) == [(3, torch.int64)]                        # [0, 6) int32 = 3 int64
    assert counted(_packed.download, (flat[1:3], flat[3:6]), torch.int64) == [(2, torch.int32), (3, torch.int32)]      # begins inside a unit
    assert counted(_packed.download, (flat[6:9], flat[9:12:2]), torch.int32) == [(3, torch.int32), (2, torch.int32)]   # a strided member
    a, b = _packed.download((flat[6:9], flat[9:12]), torch.int32)
    assert a.tolist() == [6, 7, 8] and b.tolist() == [9, 10, 11]
    for n, want in ((12, [(2, torch.int64)]), (11, [(1, torch.int64), (1, torch.int32)])):            # 11: the last unit would pass the end
        flat = torch.arange(n, dtype=torch.int32)
        tail = (flat[8:10].view(torch.int64), flat[10:11])
        assert counted(_packed.download, tail, torch.int64) == want
        got = _packed.download(tail, torch.int64)
        assert got[0].tolist() == [8 + (9 << 32)] and got[1].tolist() == [10] and got[1].dtype == np.int32


def test_pieces_begin_at_their_alignment_and_views_share_the_allocation():
    import torch
    from slnlp import _packed
    p = _packed.Packed(torch.float64, (("a", torch.int32, 3, 4), ("b", torch.float32, (2, 1), 4), ("c", torch.float64, 2, 16),
                                       ("d", torch.uint8, 5, 1, 11), ("e", torch.int32, 1, 4)), "cpu")
    assert {n: v[0] for n, v in p.at.items()} == {"a": 0, "b": 12, "c": 32, "d": 48, "e": 60} and p.flat.shape == (8,) and p.flat.dtype == torch.float64
    assert [(p.begin(n), p.end(n)) for n in p.at] == [(0, 2), (1, 3), (4, 6), (6, 8), (7, 8)]
    p.flat.view(torch.uint8).copy_(torch.arange(64, dtype=torch.uint8))
    for name, (off, dtype, shape, *_) in p.at.items():
        t = p.view(name)
        assert t.dtype == dtype and tuple(t.shape) == shape and t.data_ptr() == p.flat.data_ptr() + off, name
        assert t.untyped_storage().data_ptr() == p.flat.untyped_storage().data_ptr() and (dtype != torch.float64 or t._base is p.flat), name
    assert p.view("b", shaped=False).shape == (2,) and [tuple(t.shape) for t in p.views("e", "b")] == [(1,), (2, 1)]
    got = p.cut("b", "d")                                    # flat[1:8]: b begins 4 bytes into it
    assert list(got) == ["b", "c", "d"] and got["b"].dtype == np.float32 and got["b"].shape == (2, 1) and got["d"].tolist() == [48, 49, 50, 51, 52]
    assert got["b"].tobytes() == bytes(range(12, 20)) and got["c"].tobytes() == bytes(range(32, 48))
