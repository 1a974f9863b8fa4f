"""CPU: occlusion attribution without a GPU -- the numpy restatement (tests/attribution_ref.py) on an example worked by hand,
``ops.occlusion_variants`` against it, ``ingest.field_substitutions`` for the four composition strategies, ``metrics.attribution_report``
on the restatement's output, ``slnlp.data.DeviceRows``, the CLI key and the estimator method's own checks.  The device is held to the
restatement in tests/test_attribution_gpu.py."""
import collections
import math

import numpy as np
import pytest

import attribution_ref as ar

LN2 = math.log(2.0)


def _logp(p):
    return np.log(np.asarray(p, dtype=np.float64)).astype(np.float32)


# 3 rows, 4 classes.  Row 0 (y 0) has two variants, rows 1 (y 2) and 2 (y 5: no class) one each.
HAND_BASE = [[0.5, 0.25, 0.125, 0.125], [0.125, 0.125, 0.5, 0.25], [0.25, 0.25, 0.25, 0.25]]
HAND_VAR = [[0.25, 0.5, 0.125, 0.125],       # row 0, unit 0: classes 0 and 1 swap -- the label falls by ln 2, the arg-max flips
            [0.5, 0.25, 0.125, 0.125],       # row 0, unit 1: nothing moves
            [0.125, 0.125, 0.25, 0.5],       # row 1, unit 0: classes 2 and 3 swap
            [0.25, 0.25, 0.25, 0.25]]        # row 2, unit 0
HAND_Y = [0, 2, 5]
HAND_VARIANTS = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 0], [2, 0, 1]], dtype=np.int32)
HAND_START = np.array([0, 2, 3, 4], dtype=np.int32)


def test_hand_worked_example():
    """drop = ln(0.5) - ln(0.25) = ln 2, dp = 0.25, kl = 0.5 ln 2 + 0.25 ln(1 / 2) = 0.25 ln 2 for the two swaps; 0 where nothing
    moves.  The float32 log-probs carry the probabilities to about 1e-7."""
    from slnlp import metrics
    near = lambda a, b: np.allclose(a, b, rtol=0.0, atol=1e-6, equal_nan=True)
    nan = float("nan")
    ref = ar.attribution_ref(_logp(HAND_BASE), _logp(HAND_VAR), HAND_Y, HAND_VARIANTS, HAND_START, 2, "label")
    assert near(ref["vals"], [[LN2, 0.25, 0.25 * LN2], [0.0, 0.0, 0.0], [LN2, 0.25, 0.25 * LN2], [nan, nan, nan]])
    assert ref["ints"].tolist() == [[1, 0], [0, 0], [3, 0], [0, -1]]
    assert ref["rows_i"].tolist() == [[0, 0, 0, 2, 1, 0], [2, 2, 0, 1, 1, 0], [0, -1, -1, 0, 0, -1]]
    assert near(ref["rows_d"], [[-LN2, LN2, 0.0, LN2], [-LN2, LN2, LN2, LN2], [nan, nan, nan, 0.0]])
    want_i = np.zeros((4, 2, 3), dtype=np.int64)
    want_d = np.zeros((4, 2, 2))
    want_i[0, 0], want_i[0, 1], want_i[2, 0] = (1, 1, 0), (1, 0, 0), (1, 1, 0)
    want_d[0, 0] = want_d[2, 0] = (LN2, 0.25 * LN2)
    assert np.array_equal(ref["table_i"], want_i) and near(ref["table_d"], want_d)
    assert ref["head"].tolist() == [3, 1, 0, 0, 2, 0, 0, 0]
    assert ar.smallest_drop_gap(HAND_VARIANTS, ref["vals"], ref["ints"]) == pytest.approx(LN2, abs=1e-6)

    rep = metrics.attribution_report(ref, unit_names=["early", "late"])
    assert rep["top_unit"].tolist() == [0, 0, -1] and rep["flips"].tolist() == [1, 1, 0] and rep["units"].tolist() == [2, 1, 0]
    assert rep["base_pred"].tolist() == [0, 2, 0] and rep["target"].tolist() == [0, 2, -1]
    assert near(rep["top_drop"], [LN2, LN2, nan]) and near(rep["base_logp"], [-LN2, -LN2, nan])
    assert near(rep["per_bin"]["mean_drop"], [LN2, 0.0]) and near(rep["per_bin"]["mean_kl"], [0.25 * LN2, 0.0])
    assert rep["per_bin"]["flip_rate"].tolist() == [1.0, 0.0] and rep["per_bin"]["count"].tolist() == [2, 1]
    assert rep["per_class"]["count"].tolist() == [[1, 1], [0, 0], [1, 0], [0, 0]]
    assert np.isnan(rep["per_class"]["mean_drop"][1]).all() and np.isnan(rep["per_class"]["flip_rate"][3]).all()
    assert near(rep["per_class"]["mean_drop"][0], [LN2, 0.0]) and rep["per_class"]["flip_rate"][2, 0] == 1.0
    assert [(b, n) for b, n, _ in rep["ranking"]] == [(0, "early"), (1, "late")] and near(rep["ranking"][0][2], LN2)
    assert (rep["variants"], rep["usable"], rep["bad_labels"], rep["nonfinite_rows"], rep["invalid"], rep["total_flips"]) == (4, 3, 1, 0, 0, 2)
    with pytest.raises(ValueError, match="3 unit_names for 2 bins"):
        metrics.attribution_report(ref, unit_names=["a", "b", "c"])

    # the base row's arg-max as the target: row 2 is judged on class 0, the first of its four equal columns
    ref = ar.attribution_ref(_logp(HAND_BASE), _logp(HAND_VAR), None, HAND_VARIANTS, HAND_START, 2, "pred")
    assert ref["ints"].tolist() == [[1, 0], [0, 0], [3, 0], [0, 0]] and near(ref["vals"][3], [0.0, 0.0, 0.0])
    assert ref["rows_i"][2].tolist() == [0, 0, 0, 1, 0, 0] and ref["head"].tolist() == [4, 0, 0, 0, 2, 0, 0, 0]


def test_restatement_codes_and_special_rows():
    """-3 before -2 before -1; a row of -inf at the target in the variant gives drop = +inf with code 0, counted as nonfinite and kept
    out of every sum."""
    inf = float("inf")
    base = np.array([[0.0, -1.0, -2.0], [np.nan, 0.0, 0.0], [-1.0, -1.0, -3.0]], dtype=np.float32)
    var = np.array([[-inf, 0.0, -1.0], [0.0, 0.0, 0.0], [0.0, -inf, -inf], [-inf, -inf, -inf], [0.0, 0.0, 0.0]], dtype=np.float32)
    variants = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [2, 1, 0], [7, 0, 0]], dtype=np.int32)
    start = np.array([0, 1, 2, 4], dtype=np.int32)
    ref = ar.attribution_ref(base, var, [0, 9, 1], variants, start, 1, "label")
    assert ref["ints"].tolist() == [[1, 0], [0, -2], [0, 0], [0, -2], [-1, -3]]
    assert ref["vals"][0, 0] == inf and ref["vals"][0, 2] == inf and ref["vals"][2, 0] == inf
    assert np.isnan(ref["vals"][[1, 3, 4]]).all()
    assert ref["head"].tolist() == [2, 0, 2, 1, 1, 0, 0, 0]
    assert ref["table_i"][0, 0].tolist() == [0, 1, 1] and ref["table_i"][1, 0].tolist() == [0, 0, 1] and not ref["table_d"].any()
    assert ref["rows_i"].tolist() == [[0, 0, 0, 1, 1, -1], [0, -1, -2, 0, 0, -1], [0, 1, 0, 1, 0, -1]]


@pytest.mark.parametrize("by,width,stride,bins,fields", [("mask", 1, 1, 8, None), ("drop", 3, 1, 4, None), ("mask", 3, 2, 8, None),
                                                         ("drop", 2, 5, 64, None), ("mask", 9, 9, 1, None), ("field", 1, 1, 8, 6),
                                                         ("field", 1, 1, 8, 1)])
def test_variant_table_matches_the_restatement(by, width, stride, bins, fields):
    """Lengths 0, 1, S, above S and negative; width above a row's length; stride above the width."""
    from slnlp import ops
    S = 9
    lengths = np.array([0, 1, 2, 9, 12, -3, 5, 7, 0, 4], dtype=np.int64)
    got = ops.occlusion_variants(lengths, S, by, width=width, stride=stride, bins=bins, n_fields=fields)
    want = ar.variants_ref(lengths, S, by, width, stride, bins, fields)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    v, start = got[0], got[1]
    assert start[0] == 0 and start[-1] == len(v) and start[1] == 0 and start[9] == start[8]      # the rows of length 0 have no variant
    order = v[:, 0].astype(np.int64) * 1000 + v[:, 1]
    assert (np.diff(order) > 0).all() and v[:, 2].min() >= 0 and v[:, 2].max() < got[2]
    if by != "field":
        assert int(start[4 + 1] - start[4]) == -(-9 // stride)                                    # a length above S counts as S


def test_variant_table_by_hand_and_refusals():
    from slnlp import ops
    v, start, nb = ops.occlusion_variants(np.array([5, 0, 2]), 8, "mask", width=3, stride=2, bins=4)
    # row 0: [0, 3) [2, 5) [4, 5): centres 3 / 10, 7 / 10, 9 / 10 of the row; row 2: [0, 2): 2 / 4
    assert v.tolist() == [[0, 0, 1], [0, 1, 2], [0, 2, 3], [2, 0, 2]] and start.tolist() == [0, 3, 3, 4] and nb == 4
    empty = ops.occlusion_variants(np.zeros(3, dtype=np.int64), 8, "drop")
    assert empty[0].shape == (0, 3) and empty[1].tolist() == [0, 0, 0, 0]
    for kw, text in ((dict(by="frames"), "by='frames'"), (dict(by="mask", width=0), "width=0"), (dict(by="mask", width=9), "width=9"),
                     (dict(by="drop", stride=0), "stride=0"), (dict(by="drop", stride=9), "stride=9"), (dict(by="mask", bins=0), "bins=0"),
                     (dict(by="mask", bins=65), "bins=65"), (dict(by="field"), "n_fields=None"), (dict(by="field", n_fields=65), "n_fields=65"),
                     (dict(by="mask", bins=2.0), "bins=2.0")):
        with pytest.raises(ValueError, match="occlusion_variants: " + text):
            ops.occlusion_variants(np.array([3, 4]), 8, **kw)
    with pytest.raises(ValueError, match="lengths must be one dimension of integers"):
        ops.occlusion_variants(np.array([3.0, 4.0]), 8, "mask")
    with pytest.raises(ValueError, match="S=0"):
        ops.occlusion_variants(np.array([3]), 0, "mask")


def test_builder_restatement_by_hand():
    X = np.array([[10, 11, 12, 13, 1, 1], [20, 21, 1, 1, 1, 1]], dtype=np.int64)
    L, y = np.array([4, 2]), np.array([7, 8])
    variants = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0], [0, 2, 0], [5, 0, 0]], dtype=np.int32)
    Xo, Lo, yo = ar.occlude_ref(X, L, y, variants, "mask", width=2, stride=2, pad=1, unk=0)
    assert Xo.tolist() == [[0, 0, 12, 13, 1, 1], [10, 11, 0, 0, 1, 1], [0, 0, 1, 1, 1, 1], [1] * 6, [1] * 6, [1] * 6]
    assert Lo.tolist() == [4, 4, 2, 0, 0, 0] and yo.tolist() == [7, 7, 8, 0, 0, 0]
    Xo, Lo, yo = ar.occlude_ref(X, L, y, variants, "drop", width=2, stride=2, pad=1, unk=0)
    # row 1's only window covers the whole row: masked, not dropped
    assert Xo.tolist() == [[12, 13, 1, 1, 1, 1], [10, 11, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1], [1] * 6, [1] * 6, [1] * 6]
    assert Lo.tolist() == [2, 2, 2, 0, 0, 0] and yo.tolist() == [7, 7, 8, 0, 0, 0]
    sub = np.arange(30, dtype=np.int64).reshape(15, 2) + 100           # ids 0..14 have an entry, 20 and 21 lie outside
    Xo, Lo, yo = ar.occlude_ref(X, L, y, variants, "substitute", sub=sub)
    assert Xo.tolist() == [[120, 122, 124, 126, 1, 1], [121, 123, 125, 127, 1, 1], [20, 21, 1, 1, 1, 1], [20, 21, 1, 1, 1, 1], [1] * 6, [1] * 6]
    assert Lo.tolist() == [4, 4, 2, 2, 0, 0] and yo.tolist() == [7, 7, 8, 8, 0, 0]


FIELDS = ["orientation_dh", "movement_dh", "handshape_dh"]
_val = lambda s: None if s is None else {"value": s}
FRAMES = {"A": ("left_up", "right_down_front", "fist"), "B": (None, "right_down_front", "fist"), "C": ("left_up", None, "fist"),
          "D": ("right", "up", "flat")}


@pytest.mark.parametrize("strategy", ["all_values", "as_words", "as_words_norm", "as_sep_feat"])
def test_field_substitutions_on_a_six_word_vocabulary(strategy):
    """B is A without its orientation, C is A without its movement, D shares nothing: nulling a field of A finds B and C, every other
    nulled word is unseen and maps to <unk>; the specials map to themselves."""
    from slnlp import ingest
    compose = ingest.STRATEGIES[strategy]
    word = {k: compose([{f: _val(v) for f, v in zip(FIELDS, vals)}], FIELDS)[0] for k, vals in FRAMES.items()}
    assert len(set(word.values())) == 4
    vocab = ingest.Vocab(collections.Counter({word["A"]: 4, word["B"]: 3, word["C"]: 2, word["D"]: 1}))
    assert vocab.itos == ["<unk>", "<pad>", word["A"], word["B"], word["C"], word["D"]]
    table = ingest.field_substitutions(vocab, FIELDS, strategy)
    assert table.dtype == np.int64 and table.shape == (6, 3)
    assert table.tolist() == [[0, 0, 0], [1, 1, 1], [3, 4, 0], [3, 0, 0], [0, 4, 0], [0, 0, 0]]
    # a token that does not split into F parts maps to itself
    assert ingest.field_substitutions(vocab, FIELDS[:2], strategy).tolist() == [[v, v] for v in range(6)]
    with pytest.raises(ValueError, match="Unknown composition strategy"):
        ingest.field_substitutions(vocab, FIELDS, "as_sentences")
    with pytest.raises(ValueError, match="no fields"):
        ingest.field_substitutions(vocab, [], strategy)


def test_device_rows_and_the_hook_branch():
    import torch
    import slnlp.data as data
    from slnlp.net import NeuralNetClassifier
    ids, lengths, y = torch.zeros(3, 5, dtype=torch.int64), torch.full((3,), 5, dtype=torch.int64), torch.arange(3)
    rows = data.DeviceRows(ids, lengths, y)
    assert len(rows) == 3 and rows.ids is ids and rows.lengths is lengths and rows.y is y
    got = NeuralNetClassifier(module="model.Transformer")._device_data(rows)           # handed on as they are: no upload, no copy
    assert got[0] is ids and got[1] is lengths and got[2] is y
    for bad, text in (((ids.int(), lengths, y), "ids must be"), ((ids, lengths.float(), y), "lengths must be"), ((ids, lengths, y[:2]), "3 rows of ids"),
                      ((ids.t(), lengths, y), "ids must be"), ((ids, lengths[:, None], y), "lengths must be"), ((ids.numpy(), lengths, y), "ids must be")):
        with pytest.raises(ValueError, match="DeviceRows: " + text):
            data.DeviceRows(*bad)


def test_cli_key_is_validated():
    from slnlp import cli
    assert cli.attribution_options(None) is None and "attribution" in cli.DICT_ARGS
    assert cli.attribution_options({}) == {"by": "frame", "mode": "mask", "width": 1, "stride": 1, "bins": 8, "target": "label"}
    assert cli.attribution_options({"by": "window", "mode": "drop", "width": 3, "stride": 2, "bins": 4, "target": "pred"}) == \
        {"by": "window", "mode": "drop", "width": 3, "stride": 2, "bins": 4, "target": "pred"}
    assert cli.attribution_options({"by": "field"})["by"] == "field"
    for bad, text in (([], "expected a dict"), (False, "expected a dict"), ({"window": 3}, "unknown keys"), ({"by": "token"}, "by='token'"),
                      ({"mode": "zero"}, "mode='zero'"), ({"width": 0}, "width=0"), ({"by": "window", "width": 2.0}, "width=2.0"),
                      ({"width": True}, "width=True"), ({"stride": 0}, "stride=0"), ({"stride": "1"}, "stride='1'"), ({"bins": 0}, "bins=0"),
                      ({"bins": 65}, "bins=65"), ({"target": "gold"}, "target='gold'"), ({"width": 2}, "by='frame' occludes one frame")):
        with pytest.raises(ValueError, match="attribution.*" + text):
            cli.attribution_options(bad)


def test_attribute_checks_come_before_the_forward_pass():
    from slnlp.data import TokenDataset
    from slnlp.net import NeuralNetClassifier
    from slnlp.out_of_fold import OutOfFold
    from slnlp.ensemble import VotingEnsemble
    from slnlp.prior_shift import PriorShift
    assert VotingEnsemble.attribute is NeuralNetClassifier.attribute and PriorShift.attribute is NeuralNetClassifier.attribute
    net = NeuralNetClassifier(module="model.Transformer")
    with pytest.raises(RuntimeError, match="not initialized"):
        net.attribute(None)
    net.initialized_, net.classes_ = True, np.arange(6)
    ds = TokenDataset(np.full((4, 5), 2), np.array([5, 3, 0, 1]), np.array([0, 1, 2, 3]))
    for kw, text in ((dict(by="token"), "by='token'"), (dict(mode="zero"), "mode='zero'"), (dict(width=0), "width=0"), (dict(stride=0), "stride=0"),
                     (dict(bins=0), "bins=0"), (dict(bins=65), "bins=65"), (dict(target="gold"), "target='gold'"),
                     (dict(width=2), "by='frame' occludes one frame"), (dict(max_variants=0), "max_variants=0"),
                     (dict(by="field"), "by='field' needs substitutions"), (dict(substitutions=np.zeros((9, 2))), "substitutions are read with by='field' only"),
                     (dict(by="field", substitutions=np.zeros(9)), r"substitutions of shape \(9,\)"),
                     (dict(by="field", substitutions=np.zeros((9, 65))), r"substitutions of shape \(9, 65\)"),
                     (dict(by="window", width=6), "width=6 and stride=1 must lie in 1..5"), (dict(by="window", stride=6), "stride=6 must lie in 1..5"),
                     (dict(unit_names=["a", "b"]), "2 unit_names for 8 bins"),
                     (dict(by="field", substitutions=np.zeros((9, 3)), unit_names=["a"]), "1 unit_names for 3 bins"),
                     (dict(y=np.array([0, 1, 2])), r"y has shape \(3,\), expected \(4,\)"),
                     (dict(y=np.array([0, 1, 6, 3])), "1 of 4 labels lie outside the 6 classes")):
        with pytest.raises(ValueError, match="attribut.*" + text):
            net.attribute(ds, **kw)
    with pytest.raises(ValueError, match="attribute: no row of X has a frame to occlude"):
        net.attribute(TokenDataset(np.full((2, 5), 1), np.array([0, 0]), np.array([0, 1])))
    with pytest.raises(TypeError, match="X must be a slnlp.data.TokenDataset"):
        net.attribute([1, 2])
    net.classes_ = np.arange(4097)
    with pytest.raises(ValueError, match="attribute: 4097 classes"):
        net.attribute(ds)
    with pytest.raises(NotImplementedError, match="OutOfFold.attribute"):
        OutOfFold.attribute(object(), ds)
