"""GPU: occlusion attribution on the device -- ``slnlp_occlude_rows``, ``slnlp_attribution_rows`` and ``slnlp_attribution_summary``
through the C ABI against the numpy restatement (tests/attribution_ref.py), and ``LogProbJudge.attribute`` on fits.

The bounds.  The builder's ids, lengths and labels are integers and equal the restatement's.  The variants' arg-max and code, the
per-row counts, flips and top_unit, the table's counts and the head are integers and equal the restatement's; top_unit is honest only
where no two drops of a row nearly tie, so every case ASSERTS, as a condition on its inputs, that within a row no two finite drops of
the restatement lie closer than 1e-9.  drop, dp, kl, the base log-prob, top_drop and min_drop come from the shared fp64 row head:
within the project's 1e-12, scaled by max(1, |value|), with identical NaN / inf patterns.  A row or table sum of n terms is added in
a fixed order: within that plus n 2^-53 sum |terms| of ``math.fsum``.  The tests print the measured maxima; DESIGN.md section 4
records them."""
import numpy as np
import pytest
import torch

import attribution_ref as ar
import conformal_ref as cr

pytestmark = pytest.mark.gpu

BOUND, MARGIN = 1e-12, 1e-9
SENTINEL = 0x5A5A5A5A
SENTINEL64 = 0x5A5A5A5A5A5A5A5A


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


# ------------------------------------------------------------------------------------------------------- the builder ----
def _rows_for_builder(S, seed, Vx=30):
    """Rows of every kind of length: 0, 1, 2, 3 (a width-3 window covers them whole), S, above S, negative, and random ones; ids
    mostly inside [0, Vx), some negative and some at or above Vx."""
    rs = np.random.RandomState(seed)
    lengths = np.array([0, 1, 2, 3, S, S + 5, -2, 2 ** 40] + rs.randint(1, S + 1, size=9).tolist(), dtype=np.int64)
    n = lengths.size
    X = rs.randint(0, Vx, size=(n, S)).astype(np.int64)
    X[rs.rand(n, S) < 0.1] = -3
    X[rs.rand(n, S) < 0.1] = Vx
    X[rs.rand(n, S) < 0.05] = 2 ** 40
    y = rs.randint(0, 50, size=n).astype(np.int64)
    return X, lengths, y


def _occlude(X, L, y, variants, kind, width, stride, sub):
    """``slnlp_occlude_rows`` itself, on outputs pre-filled with a sentinel and 16 entries longer than what is written."""
    from slnlp import _lib
    lib, p = _lib.load(), _lib.ptr
    n, S = X.shape
    M = len(variants)
    Xd, Ld, yd, vd = _dev(X), _dev(L), _dev(y), _dev(variants, np.int32)
    subd = None if sub is None else _dev(sub)
    Xo = torch.full((M * S + 16,), SENTINEL64, dtype=torch.int64, device="cuda")
    Lo = torch.full((M + 16,), SENTINEL64, dtype=torch.int64, device="cuda")
    yo = torch.full((M + 16,), SENTINEL64, dtype=torch.int64, device="cuda")
    Vx, F = (0, 0) if sub is None else sub.shape
    rc = lib.slnlp_occlude_rows(p(Xd), p(Ld), p(yd), n, S, p(vd), M, ar.KINDS[kind], width, stride, 1, 0, p(subd), Vx, F, p(Xo), p(Lo), p(yo),
                                _lib.stream_ptr())
    assert rc == 0, lib.slnlp_last_error().decode()
    torch.cuda.synchronize()
    assert (Xo[M * S:] == SENTINEL64).all() and (Lo[M:] == SENTINEL64).all() and (yo[M:] == SENTINEL64).all()
    return Xo[:M * S].view(M, S).cpu().numpy(), Lo[:M].cpu().numpy(), yo[:M].cpu().numpy()


@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_builder_equals_the_restatement(S):
    X, L, y = _rows_for_builder(S, S)
    n = len(L)
    seen = 0
    for kind in ("mask", "drop"):
        for width, stride in ((1, 1), (3, 1), (3, 2), (1, 2)):
            if width > S or stride > S:
                continue
            variants, _, _ = ar.variants_ref(L, S, kind, width, stride, 8)
            # invalid ones: a row outside [0, n) on either side, a unit behind the row's end, a negative unit, any unit of a row of length 0
            extra = np.array([[n, 0, 0], [-1, 0, 0], [1, 1, 0], [4, S, 0], [4, 2 ** 31 - 1, 0], [2, -1, 0], [0, 0, 0]], dtype=np.int32)
            table = np.concatenate([variants[:5], extra, variants[5:]])
            want = ar.occlude_ref(X, L, y, table, kind, width, stride)
            got = _occlude(X, L, y, table, kind, width, stride, None)
            for g, w, what in zip(got, want, ("ids", "lengths", "labels")):
                assert np.array_equal(g, w), (S, kind, width, stride, what, np.argwhere(g != w)[:4])
            bad = slice(5, 5 + len(extra))
            assert (got[0][bad] == 1).all() and not got[1][bad].any() and not got[2][bad].any()
            if kind == "drop" and width == 3 and S >= 3:                         # rows 1, 2, 3 have lengths 1, 2, 3: their first window covers them
                whole = [j for j, (r, u, _) in enumerate(table.tolist()) if r in (1, 2, 3) and u == 0 and j not in range(5, 5 + len(extra))]
                assert len(whole) == 3 and all(got[1][j] == L[table[j, 0]] and (got[0][j, :got[1][j]] == 0).all() for j in whole)
            seen += len(table)
    rs = np.random.RandomState(S)
    sub = rs.randint(0, 30, size=(30, 4)).astype(np.int64)
    variants, _, _ = ar.variants_ref(L, S, "field", n_fields=4)
    table = np.concatenate([variants, np.array([[n, 0, 0], [1, 4, 0], [1, -1, 0], [0, 0, 0]], dtype=np.int32)])
    want = ar.occlude_ref(X, L, y, table, "substitute", sub=sub)
    got = _occlude(X, L, y, table, "substitute", 1, 1, sub)
    for g, w, what in zip(got, want, ("ids", "lengths", "labels")):
        assert np.array_equal(g, w), (S, "substitute", what, np.argwhere(g != w)[:4])
    assert (got[0][-4:] == 1).all() and not got[1][-4:].any()
    kept = X[1, 0] if not 0 <= X[1, 0] < 30 else sub[X[1, 0], 2]               # ids outside [0, Vx) pass through
    assert got[0][[j for j, (r, u, _) in enumerate(table.tolist()) if (r, u) == (1, 2)][0], 0] == kept
    print(f"S={S}: {seen + len(table)} variants of {n} rows built, ids / lengths / labels equal to the restatement")


# -------------------------------------------------------------------------------------------------- rows and summary ----
def _table(N, M, n_bins, seed, per_row=None):
    """A variant table with exactly ``M`` variants spread over ``N`` rows (some rows get none), bins drawn at random."""
    rs = np.random.RandomState(seed)
    if per_row is None:
        cuts = np.sort(rs.randint(0, M + 1, size=N - 1)) if N > 1 else np.zeros(0, dtype=np.int64)
        per_row = np.diff(np.concatenate([[0], cuts, [M]]))
    start = np.concatenate([[0], np.cumsum(per_row)]).astype(np.int32)
    rows = np.repeat(np.arange(N), per_row)
    unit = np.arange(M) - start[rows]
    return np.stack([rows, unit, rs.randint(0, n_bins, size=M)], axis=1).astype(np.int32), start


def _variant_logp(base, variants, seed, quantum=None, scale=0.7):
    """The base rows moved by noise and normalised again: drops of order 1."""
    rs = np.random.RandomState(seed)
    z = base[np.clip(variants[:, 0], 0, len(base) - 1)].astype(np.float64) + scale * rs.randn(len(variants), base.shape[1])
    z = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    if quantum:
        z = np.round(z / quantum) * quantum
    return z.astype(np.float32)


def _plain(name, N, V, M, seed, n_bins=8, ld=None, beta=1.0, target="label", quantum=None):
    base, y = cr.make_logp(N, V, seed, quantum=quantum, lean=2.0)
    variants, start = _table(N, M, n_bins, seed + 100)
    return name, base, _variant_logp(base, variants, seed + 200, quantum), y, variants, start, n_bins, ld, beta, target


def _special(target):
    inf = np.inf
    base, y = cr.make_logp(8, 9, 8, lean=2.0)
    base[0, 6] = np.nan                                                          # -2: a NaN in the base row
    base[1, 0] = inf                                                             # -2: no finite maximum
    base[2] = -inf                                                               # -2: all -inf
    base[3, y[3]] = -inf                                                         # -inf at the target: lp_b(c) = -inf
    base[4, 1] = base[4, 7] = base[4].max() + 1.0                                # two columns at the maximum
    base[5, 2], base[5, 5] = -0.0, 0.0                                           # equal values: by ascending column
    variants, start = _table(8, 40, 4, 3, per_row=np.full(8, 5))
    var = _variant_logp(np.where(np.isfinite(base), base, -3.0).astype(np.float32), variants, 5)
    var[start[6] + 0, 3] = np.nan                                                # the same four in the variant rows of a clean base row
    var[start[6] + 1, 0] = inf
    var[start[6] + 2] = -inf
    var[start[6] + 3, y[6]] = -inf                                               # drop = +inf, code 0
    var[start[3] + 1, y[3]] = -inf                                               # -inf at the target in both rows: drop NaN, code 0
    var[start[7] + 0, (y[7] + 1) % 9] = -inf                                     # -inf off the target: kl = +inf, the drop finite
    var[start[4] + 2, 0] = var[start[4] + 2, 8] = var[start[4] + 2].max() + 0.5
    return "special_" + target, base, var, y, variants, start, 4, None, 1.0, target


def _bad_labels():
    name, base, var, y, variants, start, nb, ld, beta, target = _plain("bad_labels", 20, 6, 90, 31)
    y[3], y[10], y[19] = -1, 6, 2 ** 40
    base[10, 1] = np.nan                                                         # a NaN row with a bad label: the NaN is looked at first
    variants = np.concatenate([variants, np.array([[20, 0, 0], [-1, 0, 1], [2 ** 31 - 1, 3, 2]], dtype=np.int32)])      # and three invalid variants
    var = np.concatenate([var, var[:3]])
    return name, base, var, y, variants, start, nb, ld, beta, target


def _cases():
    return [("N1_V1", np.zeros((1, 1), dtype=np.float32), np.zeros((1, 1), dtype=np.float32), np.array([0]), np.array([[0, 0, 0]], dtype=np.int32),
             np.array([0, 1], dtype=np.int32), 1, None, 1.0, "label"),
            _plain("N5_V3", 5, 3, 23, 1),
            _plain("N70_V63", 70, 63, 300, 2),                                   # one short of a wave
            _plain("N70_V64", 70, 64, 300, 3),
            _plain("N70_V65", 70, 65, 300, 4, target="pred"),
            _plain("N40_V202", 40, 202, 260, 5),                                 # the data set's classes
            _plain("N33_V129_ld136", 33, 129, 150, 6, ld=136),
            _plain("N64_V70_ties", 64, 70, 280, 7, quantum=0.25),
            _plain("N64_V70_ties_pred", 64, 70, 280, 17, quantum=0.25, target="pred"),
            _plain("beta_0.5", 70, 33, 250, 9, beta=0.5),
            _plain("beta_2.0", 70, 33, 250, 10, beta=2.0, quantum=0.25),
            _plain("M255", 30, 7, 255, 11, n_bins=2),                            # around the 256-thread tree of the table's cells
            _plain("M256", 30, 7, 256, 12, n_bins=2),
            _plain("M257", 30, 7, 257, 13, n_bins=2, target="pred"),
            _plain("M1025", 60, 5, 1025, 14, n_bins=3),
            _plain("N9000_V4", 9000, 4, 9100, 15, n_bins=2),                     # more rows and variants than waves in the grid: the stride loops wrap
            _special("label"), _special("pred"), _bad_labels()]


def _run(base, var, y, variants, start, n_bins, ld, beta, target, chunks=2, per_variant=True):
    """The two kernels through ``ops`` (ctypes calls of the C ABI), the variant rows in ``chunks`` calls at their offsets, on a
    buffer pre-filled with a sentinel; the rows' padding is NaN."""
    from slnlp import ops
    N, V = base.shape
    M = len(variants)

    def padded(z):
        full = torch.full((z.shape[0], ld or V), float("nan"), dtype=torch.float32, device="cuda")
        full[:, :V] = _dev(z)
        return full[:, :V]
    bd, vd = padded(base), padded(var)
    yd = None if y is None else _dev(y, np.int64)
    state = ops.temperature_state(beta, "cuda") if beta != 1.0 else None
    buf = ops.attribution_buffers(N, V, variants, start, n_bins, "cuda")
    buf["flat"][:buf["at"]["variants"]].fill_(SENTINEL)
    edges = np.linspace(0, M, min(chunks, M) + 1).astype(int)
    for a, b in zip(edges[:-1], edges[1:]):
        assert ops.attribution_rows(bd, vd[a:b], yd, buf, int(a), target=target, state=state) is buf
    assert ops.attribution_summary(bd, yd, buf, target=target, state=state) is buf
    return ops.attribution_download(buf, per_variant=per_variant), buf


def _same_pattern(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b))


def _excess(got, want, extra=0.0):
    """max |got - want| / (BOUND max(1, |want|) + extra) over the finite entries"""
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    bound = BOUND * np.maximum(1.0, np.abs(want)) + extra
    with np.errstate(invalid="ignore"):                      # (inf - inf where both are infinite: not among the entries looked at)
        return float((np.abs(got - want) / bound)[ok].max())


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_kernels_against_the_restatement(case):
    name, base, var, y, variants, start, n_bins, ld, beta, target = case
    N, V = base.shape
    want = ar.attribution_ref(base, var, y, variants, start, n_bins, target, beta)
    gap = ar.smallest_drop_gap(variants, want["vals"], want["ints"])
    assert gap > MARGIN, (name, gap)                                             # the condition on the inputs (change the seed, not the margin)
    got, buf = _run(base, var, y if target == "label" else None, variants, start, n_bins, ld, beta, target)
    # integers: arg-max, codes, counts, flips, top_unit, the table's counts, the head
    assert got["ints"].dtype == np.int32 and np.array_equal(got["ints"], want["ints"]), (name, np.argwhere(got["ints"] != want["ints"])[:6])
    assert np.array_equal(got["rows_i"], want["rows_i"]), (name, np.argwhere(got["rows_i"] != want["rows_i"])[:6])
    assert np.array_equal(got["table_i"], want["table_i"]), (name, np.argwhere(got["table_i"] != want["table_i"])[:6])
    assert got["head"].tolist() == want["head"].tolist(), name
    # values: identical NaN / inf patterns, the finite ones within the bound
    assert _same_pattern(got["vals"], want["vals"]), name
    assert _same_pattern(got["rows_d"], want["rows_d"]) and _same_pattern(got["table_d"], want["table_d"]), name
    e_vals = [_excess(got["vals"][:, q], want["vals"][:, q]) for q in range(3)]
    e_rows = [_excess(got["rows_d"][:, q], want["rows_d"][:, q]) for q in range(3)]
    slack = 2.0 ** -53
    rt, ct = want["row_terms"], want["cell_terms"]
    e_sum = _excess(got["rows_d"][:, 3], want["rows_d"][:, 3], rt[:, 0] * slack * rt[:, 1])
    e_tab = [_excess(got["table_d"][:, :, q], want["table_d"][:, :, q], ct[:, :, 0] * slack * ct[:, :, 1 + q]) for q in range(2)]
    # the sums alone: the restatement's fsum over the DEVICE's own terms, which leaves the order of the additions as the only difference
    own = ar.summary_ref(base, y, variants, start, n_bins, target, beta, got["vals"], got["ints"].astype(np.int64))
    assert np.array_equal(own["rows_i"], got["rows_i"]) and np.array_equal(own["table_i"], got["table_i"])
    o_sum = _excess(got["rows_d"][:, 3], own["rows_d"][:, 3], own["row_terms"][:, 0] * slack * own["row_terms"][:, 1])
    o_tab = [_excess(got["table_d"][:, :, q], own["table_d"][:, :, q], own["cell_terms"][:, :, 0] * slack * own["cell_terms"][:, :, 1 + q])
             for q in range(2)]
    top_same = got["rows_d"][:, 1].tobytes() == own["rows_d"][:, 1].tobytes() and got["rows_d"][:, 2].tobytes() == own["rows_d"][:, 2].tobytes()
    fin = np.isfinite(want["vals"])
    err = lambda q: float(np.abs(np.where(fin[:, q], got["vals"][:, q], 0.0) - np.where(fin[:, q], want["vals"][:, q], 0.0)).max())
    print(f"{name}: M {len(variants)}, smallest drop gap {gap:.3e}; max error drop {err(0):.3e} dp {err(1):.3e} kl {err(2):.3e}; error / bound: "
          f"drop {e_vals[0]:.2e} dp {e_vals[1]:.2e} kl {e_vals[2]:.2e} base_logp {e_rows[0]:.2e} top_drop {e_rows[1]:.2e} min_drop {e_rows[2]:.2e} "
          f"sum_drop {e_sum:.2e} (own terms {o_sum:.2e}) table drop {e_tab[0]:.2e} kl {e_tab[1]:.2e} (own terms {o_tab[0]:.2e} {o_tab[1]:.2e}); "
          f"head {got['head'][:5].tolist()}")
    assert max(e_vals + e_rows + [e_sum] + e_tab + [o_sum] + o_tab) <= 1.0 and top_same, name
    # without the per-variant arrays the copy ends with the rows and carries the same values
    from slnlp import ops
    lean = ops.attribution_download(buf)
    assert set(lean) == set(got) - {"vals", "ints"} and all(np.asarray(lean[q]).tobytes() == np.asarray(got[q]).tobytes() for q in lean)
    # one call for all the variant rows writes the same bits as the chunks did
    again, _ = _run(base, var, y if target == "label" else None, variants, start, n_bins, ld, beta, target, chunks=1)
    assert all(np.asarray(again[q]).tobytes() == np.asarray(got[q]).tobytes() for q in got), name
    if name == "special_label":
        s, code = start, want["ints"][:, 1]
        assert (code[s[0]:s[3]] == -2).all() and code[s[6]:s[6] + 5].tolist() == [-2, -2, -2, 0, 0]
        assert got["vals"][s[6] + 3, 0] == np.inf and np.isnan(got["vals"][s[3] + 1, 0]) and got["ints"][s[3] + 1, 1] == 0
        assert got["vals"][s[7], 2] == np.inf and np.isfinite(got["vals"][s[7], 0])
        assert got["rows_i"][:3, 2].tolist() == [-2, -2, -2] and got["rows_d"][3, 0] == -np.inf
        assert got["table_i"][:, :, 2].sum() == int((~np.isfinite(want["vals"][code == 0][:, [0, 2]]).all(axis=1)).sum()) >= 3
        assert got["ints"][s[4] + 2, 0] == 0 and got["rows_i"][4, 0] == 1 and got["rows_i"][5, 0] == int(np.argmax(base[5]))
    if name == "bad_labels":
        assert got["head"].tolist()[:4] == [int((want["ints"][:, 1] == 0).sum()), int((want["ints"][:, 1] == -1).sum()),
                                            int((want["ints"][:, 1] == -2).sum()), 3]
        assert got["ints"][-3:].tolist() == [[-1, -3]] * 3 and got["rows_i"][[3, 10, 19], 2].tolist() == [-1, -2, -1] and got["head"][1] > 0
    if name == "N1_V1":
        assert got["vals"].tolist() == [[0.0, 0.0, 0.0]] and got["rows_i"].tolist() == [[0, 0, 0, 1, 0, 0]] and got["table_i"].tolist() == [[[1, 0, 0]]]


def test_a_malformed_row_start_is_clamped_not_followed():
    """Offsets outside [0, M] and a decreasing pair read nothing they should not; entries of another row are skipped."""
    name, base, var, y, variants, start, nb, ld, beta, target = _plain("x", 6, 5, 40, 3)
    wild = np.array([-7, start[1], 2 ** 31 - 1, start[2], start[4], -1, 10 ** 9], dtype=np.int32)
    want = ar.attribution_ref(base, var, y, variants, wild, nb, target, beta)
    got, _ = _run(base, var, y, variants, wild, nb, ld, beta, target)
    assert np.array_equal(got["rows_i"], want["rows_i"]) and np.array_equal(got["table_i"], want["table_i"])
    assert got["head"].tolist() == want["head"].tolist() and _same_pattern(got["rows_d"], want["rows_d"])


def test_one_download(monkeypatch):
    from slnlp import ops
    name, base, var, y, variants, start, nb, ld, beta, target = _plain("x", 50, 37, 300, 3)
    _, buf = _run(base, var, y, variants, start, nb, ld, beta, target)
    for per_variant, a_variant in ((False, 0), (True, 32)):
        copies, real = [], torch.Tensor.cpu
        monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(t.numel() * t.element_size()) or real(t, *a, **k))
        ops.attribution_download(buf, per_variant=per_variant)
        monkeypatch.undo()
        assert len(copies) == 1 and copies[0] <= 64 + 37 * nb * 40 + 50 * 56 + 8 + 300 * a_variant, (per_variant, copies)


def test_bad_arguments_return_codes_and_messages():
    from slnlp import _lib, ops
    lib, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
    X, L, y = _dev(np.full((4, 6), 2), np.int64), _dev([6, 3, 0, 9], np.int64), _dev([0, 1, 2, 3], np.int64)
    v = _dev([[0, 0, 0], [1, 1, 1], [3, 5, 7]], np.int32)
    sub = _dev(np.zeros((5, 2)), np.int64)
    Xo, Lo, yo = torch.zeros(3, 6, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
    call = lambda *a: (lib.slnlp_occlude_rows(*a, st), lib.slnlp_last_error().decode())
    #       0     1     2     3  4  5     6  7  8  9  10 11 12      13 14 15     16     17
    good = (p(X), p(L), p(y), 4, 6, p(v), 3, 2, 1, 1, 1, 0, p(sub), 5, 2, p(Xo), p(Lo), p(yo))
    assert call(*good)[0] == 0
    for i, value, text in [(0, None, "null pointer"), (1, None, "null pointer"), (2, None, "null pointer"), (5, None, "null pointer"),
                           (15, None, "null pointer"), (16, None, "null pointer"), (17, None, "null pointer"), (12, None, "substitute needs the table"),
                           (3, 0, "n=0"), (3, 2 ** 31, "n=2147483648"), (4, 0, "S=0"), (6, 0, "M=0"), (6, 2 ** 31, "M=2147483648"),
                           (7, 3, "kind=3"), (7, -1, "kind=-1"), (14, 0, "F=0"), (14, 65, "F=65"), (13, 0, "Vx=0"), (13, 2 ** 62, "no addressable table"),
                           (5, p(v) + 2, "misaligned"), (0, p(X) + 4, "misaligned"), (16, p(Lo) + 4, "misaligned"), (12, p(sub) + 4, "misaligned"),
                           (15, p(X), "output X_out overlaps input X"), (16, p(L), "output L_out overlaps input L"),
                           (17, p(y), "output y_out overlaps input y"), (15, p(v), "output X_out overlaps input variants"),
                           (15, p(sub), "output X_out overlaps input sub"), (16, p(Xo) + 8, "outputs X_out and L_out overlap"),
                           (17, p(Lo), "outputs L_out and y_out overlap")]:
        args = list(good)
        args[i] = value
        rc, msg = call(*args)
        assert rc == 1 and "occlude_rows" in msg and text in msg, (i, value, rc, msg)
    windows = list(good)
    windows[7], windows[12] = 0, None                                            # mask: no table needed
    assert call(*windows)[0] == 0
    for i, value, text in [(8, 0, "width=0"), (8, 7, "width=7"), (9, 0, "stride=0"), (9, 7, "stride=7")]:
        args = list(windows)
        args[i] = value
        rc, msg = call(*args)
        assert rc == 1 and text in msg, (i, value, rc, msg)

    z, var = _dev(cr.make_logp(4, 3, 1)[0]), _dev(cr.make_logp(3, 3, 2)[0])
    buf = ops.attribution_buffers(4, 3, v.cpu().numpy(), np.array([0, 1, 2, 2, 3]), 8, "cuda")
    beta = ops.temperature_state(1.0, "cuda")
    vals, ints = buf["vals"], buf["ints"]
    rows = lambda *a: (lib.slnlp_attribution_rows(*a, st), lib.slnlp_last_error().decode())
    #         0     1  2       3  4     5                   6  7  8  9  10       11 12       13
    good_r = (p(z), 3, p(var), 3, p(y), p(buf["variants"]), 4, 3, 3, 0, p(beta), 0, p(vals), p(ints))
    assert rows(*good_r)[0] == 0
    for i, value, text in [(0, None, "null pointer"), (2, None, "null pointer"), (5, None, "null pointer"), (12, None, "null pointer"),
                           (13, None, "null pointer"), (4, None, "target 0 needs the labels"), (6, 0, "N=0"), (7, 0, "M=0"), (8, 0, "V=0"),
                           (8, 4097, "V=4097"), (1, 2, "ld=2 is less than V=3"), (3, 2, "ld=2 is less than V=3"), (9, 2, "target=2"),
                           (11, -1, "off=-1"), (11, 2 ** 31, "off=2147483648"), (0, p(z) + 2, "misaligned"), (2, p(var) + 2, "misaligned"),
                           (10, p(beta) + 4, "misaligned"), (12, p(vals) + 4, "misaligned"), (12, p(z), "output vals overlaps input base"),
                           (13, p(var), "output ints overlaps input var"), (13, p(buf["variants"]), "output ints overlaps input variants"),
                           (13, p(vals), "outputs vals and ints overlap")]:
        args = list(good_r)
        args[i] = value
        rc, msg = rows(*args)
        assert rc == 1 and "attribution_rows" in msg and text in msg, (i, value, rc, msg)
    args = list(good_r)
    args[4], args[9], args[10] = None, 1, None                                   # what may be null
    assert rows(*args)[0] == 0
    summ = lambda *a: (lib.slnlp_attribution_summary(*a, st), lib.slnlp_last_error().decode())
    #         0     1  2     3                   4                    5  6  7  8  9  10       11       12       13
    good_s = (p(z), 3, p(y), p(buf["variants"]), p(buf["row_start"]), 4, 3, 3, 8, 0, p(beta), p(vals), p(ints), p(buf["cell"]),
              p(buf["head"]), p(buf["table_i"]), p(buf["table_d"]), p(buf["rows_i"]), p(buf["rows_d"]))
    assert summ(*good_s)[0] == 0
    for i, value, text in [(0, None, "null pointer"), (4, None, "null pointer"), (13, None, "null pointer"), (14, None, "null pointer"),
                           (18, None, "null pointer"), (2, None, "target 0 needs the labels"), (5, 0, "N=0"), (6, 0, "0 variants"), (7, 4097, "V=4097"),
                           (8, 0, "n_bins=0"), (8, 65, "n_bins=65"), (9, 5, "target=5"), (14, p(buf["head"]) + 4, "misaligned"),
                           (13, p(ints), "output cell overlaps input ints"), (17, p(vals), "output rows_i overlaps input vals"),
                           (15, p(buf["head"]), "outputs head and table_i overlap")]:
        args = list(good_s)
        args[i] = value
        rc, msg = summ(*args)
        assert rc == 1 and "attribution_summary" in msg and text in msg, (i, value, rc, msg)
    torch.cuda.synchronize()                                                     # no sticky error: nothing faulted
    with pytest.raises(ValueError, match="occlude_rows: kind='zero'"):
        ops.occlude_rows(X, L, y, v, "zero")
    with pytest.raises(ValueError, match="occlude_rows: variants must be"):
        ops.occlude_rows(X, L, y, v.long(), "mask")
    with pytest.raises(ValueError, match="occlude_rows: substitute needs sub"):
        ops.occlude_rows(X, L, y, v, "substitute")
    with pytest.raises(ValueError, match="attribution_rows: buf must be"):
        ops.attribution_rows(z, var, y, ops.attribution_buffers(5, 3, v.cpu().numpy(), np.zeros(6), 8, "cuda"), 0)
    with pytest.raises(ValueError, match="attribution_rows: var must hold at most 2 rows"):
        ops.attribution_rows(z, var, y, buf, 1)
    with pytest.raises(ValueError, match="attribution_rows: target='gold'"):
        ops.attribution_rows(z, var, y, buf, 0, target="gold")
    with pytest.raises(ValueError, match="attribution_summary: target 'label' needs the labels"):
        ops.attribution_summary(z, None, buf)
    with pytest.raises(ValueError, match="attribution_buffers: n_bins=65"):
        ops.attribution_buffers(4, 3, v.cpu().numpy(), np.zeros(5), 65, "cuda")
    with pytest.raises(ValueError, match="attribution_buffers: variants int32"):
        ops.attribution_buffers(4, 3, np.zeros((0, 3)), np.zeros(5), 8, "cuda")


# ------------------------------------------------------------------------------------------------------ estimator ----
GRU = dict(module="model.EncoderDecoderGRUAttn", module__embedding_size=24, module__hidden_size=32, module__num_layers=2)


def make_net(ds, **kw):
    from slnlp.net import NeuralNetClassifier
    args = dict(module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y, module__batch_first=True, **GRU,
                criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1, optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05,
                max_epochs=2, batch_size=20, device="cuda", gradient_clipping={"gradient_clip_value": 0.5})
    args.update(kw)
    return NeuralNetClassifier(**args)


@pytest.fixture(scope="module")
def data():
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(60, seq_len=10, src_vocab=40, n_labels=5, seed=4, min_len=3)


@pytest.fixture(scope="module")
def fits(data):
    """Two two-epoch GRU fits, the first with a fitted temperature."""
    torch.manual_seed(41)
    a = make_net(data, calibration={"method": "temperature"}).fit(data)
    torch.manual_seed(42)
    return a, make_net(data).fit(data)


def _hook_logp(est, ds):
    """The float32 log-probs the hook hands to a consumer, as a device tensor of their own."""
    return est._forward_logp(ds, lambda logp, yd: logp.float().clone())


def _check_attribute(est, ds, beta=1.0, temperature=1.0, **kw):
    """``est.attribute`` against the restatement applied to the device's own base and variant log-probs, assembled here from the same
    ops: the variant table, the builder (held to its restatement), the hook on ``DeviceRows``."""
    from slnlp import ops
    from slnlp.data import DeviceRows
    by, mode = kw.get("by", "frame"), kw.get("mode", "mask")
    S, y = ds.ids.shape[1], np.asarray(ds.y)
    sub = kw.get("substitutions")
    if by == "field":
        variants, start, nb = ops.occlusion_variants(ds.lengths, S, "field", n_fields=sub.shape[1])
        kind = "substitute"
    else:
        variants, start, nb = ops.occlusion_variants(ds.lengths, S, mode, kw.get("width", 1), kw.get("stride", 1), kw.get("bins", 8))
        kind = mode
    pad, unk = ds.vocab_X.stoi["<pad>"], ds.vocab_X.stoi["<unk>"]
    built = ops.occlude_rows(_dev(ds.ids), _dev(ds.lengths), _dev(y, np.int64), _dev(variants), kind, width=kw.get("width", 1),
                             stride=kw.get("stride", 1), pad=pad, unk=unk, sub=None if sub is None else _dev(sub, np.int64))
    want_rows = ar.occlude_ref(ds.ids, ds.lengths, y, variants, kind, kw.get("width", 1), kw.get("stride", 1), pad, unk, sub)
    for g, w in zip(built, want_rows):
        assert np.array_equal(g.cpu().numpy(), w)                                # the device-built variant rows are the restatement's
    base = _hook_logp(est, ds).cpu().numpy()
    var = _hook_logp(est, DeviceRows(*built)).cpu().numpy()
    target = kw.get("target", "label")
    want = ar.attribution_ref(base, var, y, variants, start, nb, target, beta)
    assert ar.smallest_drop_gap(variants, want["vals"], want["ints"]) > MARGIN
    res = est.attribute(ds, per_variant=True, **kw)
    pv = res["per_variant"]
    assert np.array_equal(pv["variants"], variants) and np.array_equal(pv["row_start"], start)
    assert np.array_equal(pv["pred"], want["ints"][:, 0]) and np.array_equal(pv["code"], want["ints"][:, 1]) and not pv["code"].any()
    got_vals = np.stack([pv["drop"], pv["dp"], pv["kl"]], axis=1)
    assert _same_pattern(got_vals, want["vals"]) and max(_excess(got_vals[:, q], want["vals"][:, q]) for q in range(3)) <= 1.0
    for key, col in (("base_pred", 0), ("target", 1), ("units", 3), ("flips", 4), ("top_unit", 5)):
        assert np.array_equal(res[key], want["rows_i"][:, col]), key
    for key, col in (("base_logp", 0), ("top_drop", 1), ("min_drop", 2)):
        assert _same_pattern(res[key], want["rows_d"][:, col]) and _excess(res[key], want["rows_d"][:, col]) <= 1.0, key
    rt = want["row_terms"]
    assert _excess(res["sum_drop"], want["rows_d"][:, 3], rt[:, 0] * 2.0 ** -53 * rt[:, 1]) <= 1.0
    from slnlp import metrics
    rep = metrics.attribution_report(want, kw.get("unit_names"))
    assert np.array_equal(res["per_class"]["count"], rep["per_class"]["count"]) and np.array_equal(res["per_bin"]["count"], rep["per_bin"]["count"])
    assert np.array_equal(res["per_bin"]["flip_rate"], rep["per_bin"]["flip_rate"], equal_nan=True)
    for key in ("mean_drop", "mean_kl"):
        assert _same_pattern(res["per_bin"][key], rep["per_bin"][key]) and np.allclose(res["per_bin"][key], rep["per_bin"][key], rtol=1e-11, atol=1e-11, equal_nan=True)
        assert np.allclose(res["per_class"][key], rep["per_class"][key], rtol=1e-11, atol=1e-11, equal_nan=True)
    assert [b for b, _, _ in res["ranking"]] == [b for b, _, _ in rep["ranking"]] and res["unit_names"] == rep["unit_names"]
    assert (res["variants"], res["usable"], res["bad_labels"], res["nonfinite_rows"], res["invalid"]) == (len(variants), len(variants), 0, 0, 0)
    assert res["total_flips"] == int(want["head"][4]) and res["temperature"] == temperature and res["classes"] is est.classes_ and res["rows"] == len(ds)
    assert "per_variant" not in est.attribute(ds, **kw)
    return res, want


def test_attribute_on_a_fit(data, fits):
    hot, plain = fits
    res, want = _check_attribute(plain, data)
    print(f"GRU fit, {len(data)} rows, frame masking: {res['variants']} variants, {res['total_flips']} flips, ranking {res['ranking'][:3]}")
    _check_attribute(plain, data, by="window", mode="drop", width=2, stride=3, bins=4, target="pred")      # stride above the width
    # a fit with a temperature: at it (the device reads beta from the state), and at 1 when asked
    assert hot.temperature_ != 1.0
    _check_attribute(hot, data, beta=hot.calibration_["beta"], temperature=float(hot.temperature_))
    _check_attribute(hot, data, calibrated=False)
    # chunks of whole rows: the same table; the forward passes see other batches, so the values agree to float32 forward noise
    # (log-probs of order 1 to 10 carried in float32: 1e-4 is a hundred times their rounding)
    one = plain.attribute(data, per_variant=True)["per_variant"]
    many = plain.attribute(data, per_variant=True, max_variants=37)["per_variant"]
    assert np.array_equal(one["variants"], many["variants"]) and np.array_equal(one["code"], many["code"])
    assert np.abs(one["drop"] - many["drop"]).max() <= 1e-4
    with pytest.raises(ValueError, match="attribute: 1 of 60 labels lie outside"):
        plain.attribute(data, y=np.where(np.arange(60) == 7, len(plain.classes_), data.y))


def test_attribute_by_field_with_a_synthetic_table(data, fits):
    rs = np.random.RandomState(3)
    sub = rs.randint(0, len(data.vocab_X), size=(len(data.vocab_X), 3)).astype(np.int64)
    sub[:2] = [[0, 0, 0], [1, 1, 1]]                                             # the specials map to themselves
    res, _ = _check_attribute(fits[1], data, by="field", substitutions=sub, unit_names=["orientation", "movement", "handshape"])
    assert res["unit_names"] == ["orientation", "movement", "handshape"] and res["per_bin"]["count"].sum() == 3 * len(data)
    assert (res["units"] == 3).all() and set(res["top_unit"].tolist()) <= {0, 1, 2}


def test_attribute_on_an_ensemble_and_under_a_prior_shift(data, fits):
    import slnlp
    ens = slnlp.VotingEnsemble(list(fits))
    res, _ = _check_attribute(ens, data)
    _check_attribute(ens, data, by="window", width=2, stride=2, target="pred")
    shifted = slnlp.PriorShift(fits[1], data).set_priors(np.arange(1, len(fits[1].classes_) + 1))
    _check_attribute(shifted, data)
    with pytest.raises(NotImplementedError, match="OutOfFold.attribute"):
        slnlp.OutOfFold(list(fits), [np.arange(30), np.arange(30, 60)], dataset=data).attribute(data)


def test_planted_signal_is_found():
    """240 rows of 12 frames, six classes; the class is written only in the token at position 2, everything else is noise.  Among the
    rows the fit predicts correctly, position 2 is the most frequent top_unit -- a statement without a threshold."""
    from model.util import Vocab
    from slnlp.data import TokenDataset
    rs = np.random.RandomState(0)
    N, S, C = 240, 12, 6
    cls = rs.randint(0, C, size=N)
    X = rs.randint(8, 40, size=(N, S)).astype(np.int64)                          # noise tokens 8..39
    X[:, 2] = 2 + cls                                                            # tokens 2..7 name the class, at position 2 alone
    ds = TokenDataset(X, np.full(N, S), 2 + cls, Vocab(40), Vocab(2 + C))
    torch.manual_seed(7)
    net = make_net(ds, max_epochs=30, module__dropout=0.0).fit(ds)
    acc = float((net.predict(ds) == ds.y).mean())
    assert acc >= 0.9, acc                                                       # the condition on the input: tune epochs or seed, not the statement
    res = net.attribute(ds)
    right = res["base_pred"] == ds.y
    counts = np.bincount(res["top_unit"][right], minlength=S)
    share = counts[2] / right.sum()
    print(f"planted signal: train accuracy {acc:.3f}; position 2 is the top unit of {counts[2]} of {int(right.sum())} correctly predicted rows "
          f"({share:.3f}); counts per position {counts.tolist()}; mean drop per bin {np.round(res['per_bin']['mean_drop'], 3).tolist()}")
    assert int(np.argmax(counts)) == 2 and counts[2] > np.delete(counts, 2).max()


# ------------------------------------------------------------------------------------------------------------ CLI ----
def test_cli_writes_the_attribution_with_the_key(tmp_path):
    import csv
    import json
    import os

    from slnlp import cli
    base = {"seed": 1, "cv": 2, "max_epochs": 1, "batch_size": 16, "test_size": 0.25, "scoring": ["neg_log_loss"],
            "model": "model.EncoderDecoderGRUAttn", "model_args": {"embedding_size": 16, "hidden_size": 32, "num_layers": 1, "dropout": 0.1},
            "optimizer_args": {"momentum": 0.9}, "gradient_clipping": {"gradient_clip_value": 0.5}, "grid_args": {"lr": [0.05]},
            "dataset_args": {"synthetic": {"n": 96, "seq_len": 10, "src_vocab": 40, "n_labels": 5, "seed": 4, "min_len": 3}}}
    with pytest.raises(ValueError, match="attribution: mode='zero'"):            # before the grid search
        cli.run(cli.load_config(None, dict(base, workdir=str(tmp_path / "bad"), attribution={"mode": "zero"})))
    assert not os.path.exists(tmp_path / "bad" / "grid_search_output.json")
    work = tmp_path / "run"
    cli.run(cli.load_config(None, dict(base, workdir=str(work), attribution={"by": "window", "width": 2, "stride": 2, "bins": 4})))
    assert {"test_output.json", "test_attribution.json", "test_attribution_classes.csv"} <= set(os.listdir(work))
    got = json.load(open(work / "test_attribution.json"))
    assert set(got) == {"rows", "variants", "usable", "bad_labels", "nonfinite_rows", "invalid", "total_flips", "temperature", "options",
                        "unit_names", "ranking", "per_bin"}
    test_data, _ = cli.load_dataset(base).split(0.25, 1)
    from slnlp import ops
    variants, _, _ = ops.occlusion_variants(test_data.lengths, test_data.ids.shape[1], "mask", 2, 2, 4)
    assert (got["rows"], got["variants"], got["usable"], got["bad_labels"], got["invalid"]) == (len(test_data), len(variants), len(variants), 0, 0)
    assert got["options"] == {"by": "window", "mode": "mask", "width": 2, "stride": 2, "bins": 4, "target": "label"} and got["temperature"] == 1.0
    assert got["unit_names"] == ["0", "1", "2", "3"] and [b["count"] for b in got["per_bin"]] == np.bincount(variants[:, 2], minlength=4).tolist()
    assert sorted(b for b, _, _ in got["ranking"]) == [b["bin"] for b in got["per_bin"] if b["count"] > 0]
    assert [d for _, _, d in got["ranking"]] == sorted((d for _, _, d in got["ranking"]), reverse=True)
    lines = list(csv.reader(open(work / "test_attribution_classes.csv")))
    assert lines[0] == ["class", "name", "bin", "unit", "count", "nonfinite", "mean_drop", "mean_kl", "flip_rate"]
    assert sum(int(l[4]) + int(l[5]) for l in lines[1:]) == len(variants) and all(0.0 <= float(l[8]) <= 1.0 for l in lines[1:])
    classes = {int(l[0]) for l in lines[1:]}
    assert classes == set(np.unique(test_data.y).tolist())                       # the target is the label: a class has cells where it has rows
