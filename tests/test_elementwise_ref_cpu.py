"""CPU: the references of tests/elementwise_ref.py pinned to torch autograd / torch.nn.functional in fp64 (1e-12); every case of
tests/test_elementwise_edges_gpu.py shown to be able to fail -- a deliberately wrong restatement of the guarded branch differs
from the reference, on the GPU test's own inputs, by at least 10 x the tolerance the GPU test holds that case to; and the
argument refusals of the embedding / LayerNorm / loss entry points, which return before any launch (no device needed)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import elementwise_ref as er

PIN = 1e-12
MARGIN = 10.0


# =============================================================================================== references vs torch
@pytest.mark.parametrize("oor", [False, True])
@pytest.mark.parametrize("case", er.EMBED_BWD_CASES[:6] + [er.EMBED_FWD_SMALL + ("hot",)], ids=er.embed_case_id)
def test_embed_refs_are_autograd_of_the_gather(case, oor):
    B, S, V, E, kind = case
    ids = er.embed_ids(B, S, V, kind, oor=oor)
    tok = er.token_ids(ids)
    ok = ((tok >= 0) & (tok < V)).double()[:, None]
    table = er.rnd(V, E, seed=1).double().requires_grad_(True)
    pe = er.rnd(S, E, seed=2)
    mask = (torch.rand(S * B, E, generator=torch.Generator().manual_seed(5)) < 0.8).double()
    dx = er.rnd(S * B, E, seed=3)
    want = (torch.nn.functional.embedding(tok.clamp(0, V - 1), table) * ok * math.sqrt(E) + pe.double().repeat_interleave(B, 0)) * mask / 0.8
    want.backward(dx.double())
    got = er.embed_fwd_ref(ids, table.detach(), pe, mask=mask, p=0.2)
    assert er.err(got, want) < PIN
    assert er.row_err(er.embed_bwd_ref(ids, dx, V, mask=mask, p=0.2), table.grad) < PIN
    z = er.occurring_id(ids, V)
    dz = er.embed_bwd_ref(ids, dx, V, zero_row=z)
    assert float(dz[z].abs().max()) == 0.0
    assert kind == "equal" or float(dz.abs().max()) > 0.0
    nan = er.embed_fwd_ref(ids, table.detach(), None, nan_idx=z)
    assert torch.isnan(nan[tok == z]).all() and not torch.isnan(nan[tok != z]).any()
    assert float(er.embed_fwd_ref(ids, table.detach(), None)[ok[:, 0] == 0].abs().sum()) == 0.0      # no pe: an outside id's row is zero


@pytest.mark.parametrize("case", er.EMBED_BWD_CASES, ids=er.embed_case_id)
def test_embed_bwd_tree_is_the_scatter_add_in_float32(case):
    """The float32 restatement of the summation order agrees with the fp64 scatter-add to float32 rounding, per table row; and
    the 65536-token case really fills the combine list: id 0 owns a partial in each of its 1024 chunks."""
    B, S, V, E, kind = case
    for oor in (False, True):
        ids, dx = er.embed_bwd_inputs(case, oor=oor)
        z = er.occurring_id(ids, V) if oor else -1
        e = er.row_err(er.embed_bwd_tree(ids, dx, V, zero_row=z), er.embed_bwd_ref(ids, dx, V, zero_row=z))
        assert e < er.TOL_EMBED_BWD, e
    if kind == "every":
        tok = er.token_ids(ids).reshape(-1, 64)
        assert B * S == 65536 and tok.shape[0] == 1024 and bool((tok == 0).any(1).all())
        assert 0.35 < float((tok == 0).double().mean()) < 0.5


@pytest.mark.parametrize("rows,E", er.LN_FWD_SHAPES + er.LN_OFFSET_SHAPES + [er.LN_ZERO_VAR])
@pytest.mark.parametrize("eps", er.LN_EPS)
def test_layernorm_ref_is_torch_layer_norm_and_its_autograd(rows, E, eps):
    x, g, b, dy, _ = er.ln_inputs(rows, E, offset=er.LN_OFFSET if (rows, E) in er.LN_OFFSET_SHAPES else 0.0,
                                  const_rows=(0, rows // 2) if (rows, E) == er.LN_ZERO_VAR else ())
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, g, b))
    y = torch.nn.functional.layer_norm(xd, (E,), gd, bd, eps)
    y.backward(dy.double())
    ref = er.layernorm_ref(x, g, b, eps, dy)
    assert er.err(ref["y"], y) < PIN
    for name, grad in (("dx", xd.grad), ("dgamma", gd.grad), ("dbeta", bd.grad)):
        assert er.err(ref[name], grad) < 1e-10, name          # (dx of an offset row: rstd^2-sized terms cancel in fp64 too)
    assert er.err(ref["mean"], x.double().mean(1)) < PIN
    assert er.err(ref["rstd"], 1 / torch.sqrt(x.double().var(1, unbiased=False) + eps)) < 1e-10
    # the chunk sums add up to the column sums, and the float32 tree adds them to float32 rounding
    part = er.ln_partial_ref(dy, ref["xhat"], rows, rows)
    assert er.err(part[:, 0].sum(0), ref["dgamma"]) < PIN and er.err(part[:, 1].sum(0), ref["dbeta"]) < PIN
    tg, tb = er.ln_reduce_tree(part.float())
    assert er.err(tg, ref["dgamma"]) < 1e-5 and er.err(tb, ref["dbeta"]) < 1e-5


def test_ln_reduce_tree_order():
    """Exactly the documented order: a table whose float32 sum depends on it (2^24 swallows a 1 added after it, not before)."""
    p = torch.zeros(8, 2, 1)
    p[0, 0, 0], p[4, 0, 0], p[1, 0, 0] = 2.0 ** 24, 1.0, 1.0          # group 0: 2^24 then + 1 (lost); group 1: 1
    g, _ = er.ln_reduce_tree(p)
    assert float(g) == 2.0 ** 24 + 0.0 + 0.0 and float(g) != float(np.float32(2.0 ** 24 + 2.0))
    p[0, 0, 0], p[4, 0, 0] = 1.0, 2.0 ** 24                              # 1 then + 2^24: kept only as a rounding to even
    assert float(er.ln_reduce_tree(p)[0]) == float((np.float32(1.0) + np.float32(2.0 ** 24)) + np.float32(1.0))


LOSS_KINDS = [(B, V, "mixed") for B, V in er.LOSS_CASES] + [er.LOSS_OOR + ("oor",)]


@pytest.mark.parametrize("B,V,kind", LOSS_KINDS)
@pytest.mark.parametrize("general", [False, True])
def test_lsm_nll_ref_is_cross_entropy_on_the_log_probs(B, V, kind, general):
    logits, y, ign = er.loss_inputs(B, V, kind=kind)
    w = er.loss_weight(V) if general else None
    eps = 0.1 if general else 0.0
    x = logits.double().requires_grad_(True)
    y_torch = torch.where((y >= 0) & (y < V), y, torch.full_like(y, ign))        # torch refuses targets outside [0, V)
    for reduction in ("mean", "sum"):
        x.grad = None
        logp = torch.log_softmax(x, -1)
        loss = torch.nn.functional.cross_entropy(logp, y_torch, weight=None if w is None else w.double(), ignore_index=ign,
                                                 label_smoothing=eps, reduction=reduction)
        loss.backward()
        r_logp, r_loss, r_dl = er.lsm_nll_ref(logits, y, ign, weight=w, label_smoothing=eps, reduction=reduction)
        assert er.err(r_logp, logp) < PIN
        assert abs(float(r_loss) - float(loss.detach())) <= PIN * max(1.0, abs(float(loss.detach())))
        assert er.err(r_dl, x.grad) < PIN
    kept = (y != ign) & (y >= 0) & (y < V)
    assert float(r_dl[~kept].abs().max() if (~kept).any() else 0.0) == 0.0


def test_lsm_nll_ref_all_ignored_is_nan_and_no_gradient():
    logits, y, ign = er.loss_inputs(*er.LOSS_ALL_IGNORED, kind="all_ignored")
    _, loss, dl = er.lsm_nll_ref(logits, y, ign)
    want = torch.nn.functional.cross_entropy(torch.log_softmax(logits.double(), -1), y, ignore_index=ign)
    assert math.isnan(float(loss)) and math.isnan(float(want)) and float(dl.abs().max()) == 0.0


# ====================================================================== every guard can fail: wrong restatements, 10 x the bound
def test_one_pass_variance_misses_the_forward_bound_on_the_offset_input():
    """x = 100 + randn: float32 two-pass statistics stay inside 2e-5 of the output maximum, E[x^2] - mean^2 does not by far."""
    for rows, E in er.LN_OFFSET_SHAPES:
        x, g, b, _, _ = er.ln_inputs(rows, E, offset=er.LN_OFFSET)
        ref = er.layernorm_ref(x, g, b)["y"]
        two, one = er.err(er.layernorm_fwd_f32(x, g, b), ref), er.err(er.layernorm_fwd_f32(x, g, b, one_pass=True), ref)
        print(f"offset {er.LN_OFFSET} ({rows}, {E}): two-pass {two:.2e}, one-pass {one:.2e}")
        assert two < er.TOL_LN_FWD and one >= MARGIN * er.TOL_LN_FWD


def test_zero_mean_inputs_cannot_tell_one_pass_from_two_pass():
    """... which is why the offset case exists: on the zero-mean shapes the one-pass forward is inside the bound."""
    x, g, b, _, _ = er.ln_inputs(9, 512)
    assert er.err(er.layernorm_fwd_f32(x, g, b, one_pass=True), er.layernorm_ref(x, g, b)["y"]) < er.TOL_LN_FWD


@pytest.mark.parametrize("case", [c for c in er.EMBED_BWD_CASES if c[3] > 256], ids=er.embed_case_id)
def test_a_skipped_column_trip_shows_in_every_wide_embedding_case(case):
    B, S, V, E, _ = case
    ids, dx = er.embed_bwd_inputs(case)
    ref = er.embed_bwd_ref(ids, dx, V)
    for limit in range(256, E, 256):                       # the columns of trip c0 = limit and beyond never written
        assert er.row_err(er.embed_bwd_tree(ids, dx, V, col_limit=limit), ref) >= MARGIN * er.TOL_EMBED_BWD
    if E % 256:                                            # the last trip's guard c < E: its live lanes dropped
        assert er.row_err(er.embed_bwd_tree(ids, dx, V, col_limit=E - E % 256), ref) >= MARGIN * er.TOL_EMBED_BWD


@pytest.mark.parametrize("case", [c for c in er.EMBED_BWD_CASES if (c[0] * c[1]) % 64], ids=er.embed_case_id)
def test_a_dropped_last_chunk_shows_in_every_ragged_embedding_case(case):
    B, S, V, E, _ = case
    ids, dx = er.embed_bwd_inputs(case)
    M = B * S
    wrong = er.embed_bwd_tree(ids, dx, V, n_tokens=M - M % 64)
    assert er.row_err(wrong, er.embed_bwd_ref(ids, dx, V)) >= MARGIN * er.TOL_EMBED_BWD


def test_a_wrong_rare_row_hides_under_the_hot_row_but_not_from_the_row_metric():
    """(50, 48, 300, 1024): id 0's row sums ~1000 tokens, a rare id's row is one token.  An error of 2e-4 of the rare row is
    20 x the bound by the row metric and inside the bound against the tensor maximum."""
    case = er.EMBED_BWD_CASES[2]
    B, S, V, E, _ = case
    ids, dx = er.embed_bwd_inputs(case)
    ref = er.embed_bwd_ref(ids, dx, V)
    counts = torch.bincount(er.token_ids(ids), minlength=V)
    rare = int((counts == 1).nonzero()[0])
    assert int(counts[0]) > 800
    wrong = ref.clone()
    wrong[rare] *= 1.0 + 2e-4
    assert er.err(wrong, ref) < er.TOL_EMBED_BWD
    assert er.row_err(wrong, ref) >= MARGIN * er.TOL_EMBED_BWD


@pytest.mark.parametrize("rows_enc", [r for r in er.LN_TABLE_SHORT_ENC if r % 8])
def test_dropped_tail_rows_of_the_8_row_loop_show_in_the_table_cases(rows_enc):
    E = er.LN_TABLE_E
    x, g, b, dy, _ = er.ln_inputs(er.LN_TABLE_ENC, E, seed=10)
    xhat = er.layernorm_ref(x, g, b)["xhat"]
    ref = er.ln_partial_ref(dy, xhat, rows_enc, er.LN_TABLE_ENC)
    wrong = er.ln_partial_ref(dy, xhat, rows_enc, er.LN_TABLE_ENC, drop_tail_of=8)
    last = (rows_enc - 1) // 16
    assert er.err(wrong[last], ref[last]) >= MARGIN * er.TOL_LN_BWD


def test_the_table_cases_cover_a_chunk_of_exactly_8_rows_and_every_tail():
    tails = {r: (r - (r - 1) // 16 * 16) for r in er.LN_TABLE_SHORT_ENC}       # rows in the last chunk
    assert tails == {23: 7, 24: 8, 25: 9, 31: 15}


@pytest.mark.parametrize("rows,full_rows,E", er.LN_SHORT_CASES)
def test_unwritten_trailing_chunks_show_in_the_short_batch_cases(rows, full_rows, E):
    """A NaN-prefilled partial table whose trailing chunks stay unwritten reduces to NaN; one whose last live chunk is dropped
    misses dgamma by far more than the bound."""
    x, g, b, dy, _ = er.ln_inputs(rows, E, seed=20)
    ref = er.layernorm_ref(x, g, b, dy=dy)
    part = er.ln_partial_ref(dy, ref["xhat"], rows, full_rows)
    nblk, live = -(-full_rows // 16), -(-rows // 16)
    assert part.shape[0] == nblk and live < nblk and float(part[live:].abs().max()) == 0.0
    unwritten = part.clone().float()
    unwritten[live:] = math.nan
    assert er.err(er.ln_reduce_tree(unwritten)[0], ref["dgamma"]) == math.inf
    dropped = part.clone().float()
    dropped[live - 1] = 0.0
    assert er.err(er.ln_reduce_tree(dropped)[0], ref["dgamma"]) >= MARGIN * er.TOL_LN_BWD
    assert er.err(er.ln_reduce_tree(part.float())[0], ref["dgamma"]) < er.TOL_LN_BWD


@pytest.mark.parametrize("B,V,kind", [c for c in LOSS_KINDS if c[0] >= 3])
def test_counting_ignored_rows_in_the_mean_shows_in_every_case_that_has_them(B, V, kind):
    logits, y, ign = er.loss_inputs(B, V, kind=kind)
    _, loss, dl = er.lsm_nll_ref(logits, y, ign)
    _, loss_w, dl_w = er.lsm_nll_ref(logits, y, ign, count_ignored=True)
    assert er.err(dl_w, dl) >= MARGIN * er.TOL_LOSS_GRAD
    assert abs(float(loss_w) - float(loss)) >= MARGIN * 1e-6 * abs(float(loss))


def test_a_softmax_without_its_max_overflows_on_the_saturated_case():
    B, V = er.LOSS_SATURATED
    logits, y, ign = er.loss_inputs(B, V, scale=30.0)
    assert float(logits.max()) > 89.0                      # exp overflows float32 past 88.7
    logp, loss, dl = er.lsm_nll_ref(logits, y, ign)
    lp32, loss32, dl32 = er.lsm_nll_f32(logits, y, ign)
    e_logp, e_dl = er.err(lp32, logp), er.err(dl32, dl)
    print(f"saturated ({B}, {V}) float32 restatement: logp {e_logp:.2e}, dlogits {e_dl:.2e}")
    assert e_logp < er.TOL_LOGP and e_dl < er.TOL_LOSS_GRAD      # the kernel's formulas in float32 keep the bounds here
    lpw, _, dlw = er.lsm_nll_f32(logits, y, ign, subtract_max=False)
    assert er.err(lpw, logp) >= MARGIN * er.TOL_LOGP and er.err(dlw, dl) >= MARGIN * er.TOL_LOSS_GRAD


# ==================================================================================== refusals: codes and messages, no launch
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    return _lib.load()


INVALID = 1                                                  # SLNLP_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def p():
    buf = (C.c_float * 16)()
    yield C.cast(buf, C.c_void_p).value                      # any non-null address: nothing below gets as far as reading it


def test_layernorm_entry_points_refuse_rows_they_cannot_hold(lib, p):
    nblk = C.c_int32(0)

    def fwd(E, x=p, rows=3):
        return lib.slnlp_layernorm_fwd(x, p, p, rows, E, 1e-5, p, p, None)

    def fwd_ex(E, x=p, rows=3, hi=None, lo=None):
        return lib.slnlp_layernorm_fwd_ex(x, p, p, rows, E, 1e-5, p, p, hi, lo, None)

    def bwd(E, dy=p, rows=3):
        return lib.slnlp_layernorm_bwd(dy, p, p, p, rows, E, None, p, None, 0.0, 0, None, p, C.byref(nblk), None)

    def bwd_ex(E, dy=p, rows=3, full_rows=0, planes=(None, None, None, None), drop_p=0.0):
        return lib.slnlp_layernorm_bwd_ex(dy, p, p, p, rows, E, None, p, None, drop_p, 0, None, None, None, full_rows, *planes, None)

    for call in (fwd, fwd_ex, bwd, bwd_ex):
        assert call(1028) == INVALID and b"1024" in lib.slnlp_last_error()          # E > 4 float4 per lane
        assert call(6) == INVALID and b"E" in lib.slnlp_last_error()                # E % 4 != 0
        assert call(0) == INVALID and call(8, rows=0) == INVALID
        assert call(8, None) == INVALID and b"null" in lib.slnlp_last_error()
    assert fwd_ex(8, hi=p) == INVALID and b"planes" in lib.slnlp_last_error()
    assert bwd_ex(8, planes=(p, None, None, None)) == INVALID and b"planes" in lib.slnlp_last_error()
    assert bwd_ex(8, planes=(None, None, None, p)) == INVALID and b"planes" in lib.slnlp_last_error()
    assert bwd_ex(8, full_rows=-1) == INVALID and b"full_rows" in lib.slnlp_last_error()
    assert bwd_ex(8, drop_p=0.2) == INVALID and b"dropout" in lib.slnlp_last_error()       # dropout without its rng


def test_ln_param_partial_and_reduce_refuse_before_they_launch(lib, p):
    from slnlp import _lib
    assert C.sizeof(_lib.LnPartialEntry) == 40               # slnlp_ln_partial_entry: four pointers, dec, pad

    def partial(E=128, n=1, tab=p, rows=(4, 2), full=(4, 2)):
        return lib.slnlp_ln_param_partial(tab, n, E, rows[0], rows[1], full[0], full[1], None)

    assert partial(E=1028) == INVALID and b"1024" in lib.slnlp_last_error()
    assert partial(E=6) == INVALID and partial(E=0) == INVALID
    assert partial(tab=None) == INVALID and b"null" in lib.slnlp_last_error()
    assert partial(n=0) == INVALID and partial(n=65536) == INVALID and b"entries" in lib.slnlp_last_error()
    assert partial(rows=(5, 2)) == INVALID and b"rows" in lib.slnlp_last_error()          # more rows than the full batch
    assert partial(rows=(4, -1)) == INVALID
    assert lib.slnlp_ln_param_reduce(None, 1, 128, None) == INVALID and lib.slnlp_ln_param_reduce(p, 0, 128, None) == INVALID


def test_embed_entry_points_refuse_before_they_launch(lib, p):
    def fwd(B=2, S=3, E=8, V=5, ids=p, ld=3, ex=False, hi=None, lo=None, drop_p=0.0):
        if ex:
            return lib.slnlp_embed_fwd_ex(ids, ld, B, S, E, V, p, None, p, 1.0, drop_p, 0, None, -1, hi, lo, None, None)
        return lib.slnlp_embed_fwd(ids, ld, B, S, E, V, p, None, p, 1.0, drop_p, 0, None, -1, None)

    def bwd(B=2, S=3, E=8, V=5, ids=p, ld=3, ex=False, scratch=p, drop_p=0.0):
        if ex:
            return lib.slnlp_embed_bwd_ex(ids, ld, B, S, E, V, p, p, 1.0, -1, drop_p, 0, None, scratch, None, None)
        return lib.slnlp_embed_bwd(ids, ld, B, S, E, V, p, p, 1.0, -1, drop_p, 0, None, scratch, None)

    for ex in (False, True):
        for call in (fwd, bwd):
            assert call(E=6, ex=ex) == INVALID and b"shape" in lib.slnlp_last_error()
            assert call(E=0, ex=ex) == INVALID and call(B=0, ex=ex) == INVALID and call(V=0, ex=ex) == INVALID
            assert call(ids=None, ex=ex) == INVALID and b"null" in lib.slnlp_last_error()
            assert call(drop_p=0.2, ex=ex) == INVALID and b"dropout" in lib.slnlp_last_error()
            assert call(drop_p=1.0, ex=ex) == INVALID
        assert bwd(B=1, S=65537, ld=65537, ex=ex) == INVALID and b"65536" in lib.slnlp_last_error()      # one token too many
        assert bwd(B=257, S=256, ld=256, ex=ex) == INVALID and b"tokens" in lib.slnlp_last_error()
        assert bwd(scratch=None, ex=ex) == INVALID and b"null" in lib.slnlp_last_error()
    assert fwd(ld=2, ex=True) == INVALID and b"ld_ids" in lib.slnlp_last_error()
    assert bwd(ld=2, ex=True) == INVALID and b"ld_ids" in lib.slnlp_last_error()
    assert fwd(ex=True, hi=p) == INVALID and fwd(ex=True, lo=p) == INVALID and b"planes" in lib.slnlp_last_error()


def test_loss_entry_points_refuse_before_they_launch(lib, p):
    def nll(B=4, V=7, ld=7, ldd=7, logits=p, rows=p, ex=False, eps=0.0, red=0):
        if ex:
            return lib.slnlp_lsm_nll_ex(logits, ld, p, B, V, 1, None, eps, red, p, p, p, ldd, rows, None)
        return lib.slnlp_lsm_nll(logits, ld, p, B, V, 1, p, p, p, ldd, rows, None)

    for ex in (False, True):
        assert nll(B=1025, ex=ex) == INVALID and b"B=1025" in lib.slnlp_last_error()       # one wave's row table holds 1024 rows
        assert nll(B=0, ex=ex) == INVALID and nll(V=0, ex=ex) == INVALID
        assert nll(ld=6, ex=ex) == INVALID and b"shape" in lib.slnlp_last_error()          # ld_logits < V
        assert nll(ldd=6, ex=ex) == INVALID and b"ld_dlogits" in lib.slnlp_last_error()
        assert nll(logits=None, ex=ex) == INVALID and b"null" in lib.slnlp_last_error()
        assert nll(rows=None, ex=ex) == INVALID and b"null" in lib.slnlp_last_error()
    assert nll(ex=True, eps=1.5) == INVALID and b"label_smoothing" in lib.slnlp_last_error()
    assert nll(ex=True, red=2) == INVALID
    assert lib.slnlp_lsm_bwd(p, p, 4, 7, p, 6, None) == INVALID and lib.slnlp_lsm_bwd(None, p, 4, 7, p, 7, None) == INVALID
    assert lib.slnlp_lsm_bwd(p, p, 0, 7, p, 7, None) == INVALID
