"""GPU: the kernels of csrc/elementwise.hip (embedding gather and scatter-add, LayerNorm forward / backward and its two-level
(dgamma, dbeta) reduction, the log-softmax / NLL criterion) and the optimizer step of csrc/update.hip against the plain fp64
references of tests/elementwise_ref.py, at the smallest shapes that reach each branch of their launchers (the case table lives
there, and tests/test_elementwise_ref_cpu.py shows that every case can fail).  Bounds are the project's own, relative to the
reference tensor's maximum: 1e-6 embedding forward, 1e-5 embedding backward (per table row, against the row's own maximum) and
loss gradients, 2e-5 LayerNorm forward, 5e-5 LayerNorm backward.  Where the summation order is documented and the sums are plain
adds (the embedding backward without dropout, ln_param_reduce) the result is also held to the float32 restatement bit for bit.

SLNLP_ELEMENTWISE_PROFILE=<path>: also write the largest measured error per family and output there
(profiles/elementwise_edges.json)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import elementwise_ref as er
from kernel_refs import planes_are_the_split_of

pytestmark = pytest.mark.gpu

SEED, STEP = 4, 0
P_DROP = 0.2
MEASURED, BOUNDS = {}, {}


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    yield o
    path = os.environ.get("SLNLP_ELEMENTWISE_PROFILE")
    if path and MEASURED:
        doc = {"what": "tests/test_elementwise_edges_gpu.py on an MI355X: max |kernel - fp64 reference| / max |reference| per family and "
                       "output, the maximum over all cases (embed_bwd: per table row, against the row's own maximum)",
               "bounds": {k: dict(sorted(d.items())) for k, d in sorted(BOUNDS.items())},
               "max_error_over_all_cases": {k: {n: float(f"{v:.3e}") for n, v in sorted(d.items())} for k, d in sorted(MEASURED.items())}}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def held(family, name, got, ref, bound, metric=er.err):
    """Measure, print, record, then assert: the error of `got` against `ref` stays under `bound`."""
    e = metric(got, ref)
    print(f"{family} {name}: {e:.2e} (bound {bound:.1e})")
    d = MEASURED.setdefault(family, {})
    d[name] = max(d.get(name, 0.0), e) if math.isfinite(e) else math.inf
    BOUNDS.setdefault(family, {})[name] = bound
    assert e < bound, (family, name, e, bound)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def exactly_zero(t):
    """Every element equals zero (either sign: 0 * x is -0 for a negative x); a NaN does not."""
    return bool((t == 0).all())


def all_nan(t):
    return bool(torch.isnan(t).all())


def view_of(ids):
    """The ids on the device as a column view of a wider matrix: ld_ids = S + ID_PAD."""
    return er.padded(ids).cuda()[:, :ids.shape[1]]


# ============================================================================================================ embedding forward
@pytest.mark.parametrize("p", [0.0, P_DROP])
def test_embed_fwd_grid_stride(ops, p):
    """540672 float4 on a grid clamped at 2048 x 256 = 524288 threads: the first 16384 threads make a second trip."""
    from slnlp.tf_engine import positional_table
    B, S, V, E = er.EMBED_FWD_STRIDE
    assert B * S * E // 4 > 2048 * 256
    ids = er.embed_ids(B, S, V, "hot")
    table, pe = er.rnd(V, E, seed=1), positional_table(S, E)
    rng = ops.make_rng(seed=SEED, step=STEP)
    mask = ops.dropout_mask(S * B, E, p, 1, rng).cpu() if p else None
    out, planes, keep = ops.embed_fwd_ex(ids.cuda(), table.cuda(), pe.cuda(), B=B, S=S, drop_p=p, drop_site=1, rng=rng if p else None,
                                         want_planes=True, want_keep=True)
    held("embed_fwd", "out", out, er.embed_fwd_ref(ids, table, pe, mask=mask, p=p), er.TOL_EMBED_FWD)
    assert planes_are_the_split_of(planes, out)
    if p:           # each float4's recorded 4 bits are the bits of the mask
        want = (mask.reshape(-1, 4).to(torch.uint8) * torch.tensor([1, 2, 4, 8], dtype=torch.uint8)).sum(1).to(torch.uint8)
        assert torch.equal(keep.cpu(), want)
        assert 0.15 < 1.0 - float(mask.mean()) < 0.25
    else:
        assert int(keep.max()) == 0                  # without dropout nothing is recorded


@pytest.mark.parametrize("p", [0.0, P_DROP])
def test_embed_fwd_ids_outside_the_table_no_pe_padded_ids_nan_row(ops, p):
    B, S, V, E = er.EMBED_FWD_SMALL
    ids = er.embed_ids(B, S, V, "hot", oor=True)
    tok = er.token_ids(ids)
    assert {-1, V, V + 5} <= set(tok.tolist())
    table = er.rnd(V, E, seed=1)
    rng = ops.make_rng(seed=SEED, step=STEP)
    mask = ops.dropout_mask(S * B, E, p, 2, rng).cpu() if p else None
    for nan_idx in (-1, er.occurring_id(ids, V)):
        out, planes, _ = ops.embed_fwd_ex(view_of(ids), table.cuda(), None, B=B, S=S, drop_p=p, drop_site=2, rng=rng if p else None,
                                          nan_idx=nan_idx, want_planes=nan_idx < 0)
        ref = er.embed_fwd_ref(ids, table, None, mask=mask, p=p, nan_idx=nan_idx)
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(out.cpu()), nan) and bool(nan.any()) == (nan_idx >= 0)
        held("embed_fwd", "out", torch.where(nan, 0.0, out.cpu().double()), torch.where(nan, 0.0, ref), er.TOL_EMBED_FWD)
        outside = (tok < 0) | (tok >= V)                 # (never the NaN id, which occurs in the table)
        assert same_bits(out.cpu()[outside].abs(), torch.zeros(int(outside.sum()), E))     # no pe: an outside id's row is exactly zero
        if planes:
            assert planes_are_the_split_of(planes, out)


# =========================================================================================================== embedding backward
def _mask(ops, M, E, p, site, rng):
    return ops.dropout_mask(M, E, p, site, rng).cpu() if p else None


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("case", er.EMBED_BWD_CASES, ids=er.embed_case_id)
def test_embed_bwd_chunk_and_combine(ops, case, p):
    B, S, V, E, kind = case
    M, site = B * S, 7
    assert M > 64                                        # the chunk + combine launches, whatever the mask
    rng = ops.make_rng(seed=SEED, step=STEP)
    kw = dict(B=B, S=S, V=V, drop_p=p, drop_site=site, rng=rng if p else None)
    mask = _mask(ops, M, E, p, site, rng)
    ids, dx = er.embed_bwd_inputs(case)
    dxd = dx.cuda()
    # plain ids: fp64 per row, untouched rows exactly zero over a NaN-filled table, run to run, the documented order's bits
    nan_table = lambda: torch.full((V, E), math.nan, device="cuda")
    got = ops.embed_bwd_ex(ids.cuda(), dxd, out=nan_table(), **kw)
    held("embed_bwd", "dtable", got, er.embed_bwd_ref(ids, dx, V, mask=mask, p=p), er.TOL_EMBED_BWD, er.row_err)
    unused = torch.ones(V, dtype=torch.bool)
    unused[er.token_ids(ids)] = False
    assert bool(unused.any()) or V <= 30
    assert same_bits(got.cpu()[unused], torch.zeros(int(unused.sum()), E))
    assert same_bits(got, ops.embed_bwd_ex(ids.cuda(), dxd, out=nan_table(), **kw))
    if not p:
        assert torch.equal(got.cpu(), er.embed_bwd_tree(ids, dx, V))
    # ids outside the table mixed in, a padded id matrix, a zero_row that occurs
    ids = er.embed_ids(B, S, V, kind, oor=True)
    z = er.occurring_id(ids, V)
    got = ops.embed_bwd_ex(view_of(ids), dxd, out=nan_table(), zero_row=z, **kw)
    held("embed_bwd", "dtable_outside_ids_zero_row", got, er.embed_bwd_ref(ids, dx, V, zero_row=z, mask=mask, p=p), er.TOL_EMBED_BWD,
         er.row_err)
    assert same_bits(got[z], torch.zeros(E)) and not bool(torch.isnan(got).any())
    if not p:
        assert torch.equal(got.cpu(), er.embed_bwd_tree(ids, dx, V, zero_row=z))
    else:           # the keep bits the forward recorded give the backward that draws the lots again, bit for bit
        _, _, keep = ops.embed_fwd_ex(view_of(ids), er.rnd(V, E, seed=1).cuda(), None, B=B, S=S, drop_p=p, drop_site=site, rng=rng,
                                      want_keep=True)
        assert same_bits(got, ops.embed_bwd_ex(view_of(ids), dxd, out=nan_table(), zero_row=z, keep_mask=keep, **kw))


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("B,S,V,E", er.EMBED_BWD_ONE_CHUNK)
def test_embed_bwd_single_launch_has_the_bits_of_chunk_and_combine(ops, B, S, V, E, p):
    """At most 64 tokens: without a keep mask the single launch, with one the chunk + combine launches -- the same bits, as the
    comment on embed_bwd_small says."""
    M, site = B * S, 7
    assert M <= 64
    ids, dx = er.embed_ids(B, S, V, "hot"), er.rnd(M, E, seed=3)
    rng = ops.make_rng(seed=SEED, step=STEP)
    kw = dict(B=B, S=S, V=V, drop_p=p, drop_site=site, rng=rng if p else None)
    _, _, keep = ops.embed_fwd_ex(ids.cuda(), er.rnd(V, E, seed=1).cuda(), None, B=B, S=S, drop_p=p, drop_site=site,
                                  rng=rng if p else None, want_keep=True)
    single = ops.embed_bwd_ex(ids.cuda(), dx.cuda(), out=torch.full((V, E), math.nan, device="cuda"), **kw)
    chunked = ops.embed_bwd_ex(ids.cuda(), dx.cuda(), out=torch.full((V, E), math.nan, device="cuda"), keep_mask=keep, **kw)
    assert torch.equal(single, chunked)
    held("embed_bwd", "dtable_one_chunk", chunked, er.embed_bwd_ref(ids, dx, V, mask=_mask(ops, M, E, p, site, rng), p=p),
         er.TOL_EMBED_BWD, er.row_err)
    if not p:
        assert torch.equal(single.cpu(), er.embed_bwd_tree(ids, dx, V))


# ============================================================================================================ LayerNorm forward
def _stats(ref):
    return torch.stack([ref["mean"], ref["rstd"]], 1).float()


@pytest.mark.parametrize("eps", er.LN_EPS)
@pytest.mark.parametrize("rows,E,offset", [s + (0.0,) for s in er.LN_FWD_SHAPES] + [s + (er.LN_OFFSET,) for s in er.LN_OFFSET_SHAPES])
def test_layernorm_fwd_boundaries_stats_and_planes(ops, rows, E, offset, eps):
    x, g, b, _, _ = er.ln_inputs(rows, E, offset=offset)
    ref = er.layernorm_ref(x, g, b, eps)
    y, stats, planes = ops.layernorm_fwd_ex(x.cuda(), g.cuda(), b.cuda(), eps, want_planes=True)
    fam = "layernorm_fwd_offset" if offset else "layernorm_fwd"
    held(fam, "y", y, ref["y"], er.TOL_LN_FWD)
    held(fam, "mean", stats[:, 0], ref["mean"], er.TOL_STATS)
    held(fam, "rstd", stats[:, 1], ref["rstd"], er.TOL_STATS)
    assert planes_are_the_split_of(planes, y)
    y2, stats2 = ops.layernorm_fwd(x.cuda(), g.cuda(), b.cuda(), eps)
    assert same_bits(y, y2) and same_bits(stats, stats2)


@pytest.mark.parametrize("eps", er.LN_EPS)
def test_layernorm_fwd_constant_rows(ops, eps):
    """Rows of the constant 2: the mean of E twos is exact, every deviation is zero, so y is beta and rstd is 1 / sqrt(eps) as
    float32 computes it (a correctly rounded square root, then a correctly rounded division)."""
    for rows, E in er.LN_FWD_SHAPES:
        _, g, b, _, _ = er.ln_inputs(rows, E)
        y, stats, _ = ops.layernorm_fwd_ex(torch.full((rows, E), 2.0, device="cuda"), g.cuda(), b.cuda(), eps)
        assert same_bits(y, b.expand(rows, E))
        assert same_bits(stats[:, 0], torch.full((rows,), 2.0))
        rstd = np.float32(1) / np.sqrt(np.float32(eps))
        assert same_bits(stats[:, 1], torch.full((rows,), float(rstd)))


# =========================================================================================================== LayerNorm backward
def _reduce(ops, partial, nblk, E):
    dg, db = torch.full((E,), math.nan, device="cuda"), torch.full((E,), math.nan, device="cuda")
    ops.ln_param_reduce([dict(partial=partial, dgamma=dg, dbeta=db, nblk=nblk, E=E)], E)
    return dg, db


@pytest.mark.parametrize("add", [True, False], ids=["add", "noadd"])
@pytest.mark.parametrize("name,rows,E", er.LN_BWD_CASES, ids=[f"{n}-{r}x{e}" for n, r, e in er.LN_BWD_CASES])
def test_layernorm_bwd_every_kernel_instance(ops, name, rows, E, add):
    fused, unfused4 = name.endswith("f") or "chunk32" in name, name.endswith("g4")
    assert (rows >= 1024) == (fused or unfused4) and name.startswith("u%d" % (1 if E <= 256 else 2 if E <= 512 else 4))
    x, g, b, dy, addt = er.ln_inputs(rows, E)
    ref = er.layernorm_ref(x, g, b, dy=dy)
    want_dx = ref["dx"] + addt.double() if add else ref["dx"]
    dev = [t.cuda() for t in (dy, x, g)] + [_stats(ref).cuda()]
    kw = dict(add_to_dx=addt.cuda() if add else None)
    chunk = er.ln_partial_chunk(rows)
    nblk = -(-rows // chunk)
    assert ("chunk32" in name) == (chunk == 32)
    partial = None if unfused4 else torch.full((nblk + 2, 2, E), math.nan, device="cuda")
    fam = "layernorm_bwd_" + ("fused" if fused else "g4" if unfused4 else "g1")
    rng = ops.make_rng(seed=SEED, step=STEP)
    site = 11
    # dx, the dropout copy under p = 0.2, the chunk sums and their reduction
    r = ops.layernorm_bwd_ex(*dev, want_drop=True, drop_p=P_DROP, drop_site=site, rng=rng, partial=partial, **kw)
    mask = ops.dropout_mask(rows, E, P_DROP, site, rng).cpu().double()
    held(fam, "dx", r["dx"], want_dx, er.TOL_LN_BWD)
    held(fam, "dx_drop", r["dx_drop"], want_dx * mask / (1 - P_DROP), er.TOL_LN_BWD)
    assert r["nblk"] == nblk
    if partial is not None:
        assert all_nan(partial[nblk:]) and not bool(torch.isnan(partial[:nblk]).any())
        held(fam, "partial", partial[:nblk], er.ln_partial_ref(dy, ref["xhat"], rows, rows), er.TOL_LN_BWD)
        dg, db = _reduce(ops, partial, nblk, E)
        held(fam, "dgamma", dg, ref["dgamma"], er.TOL_LN_BWD)
        held(fam, "dbeta", db, ref["dbeta"], er.TOL_LN_BWD)
        tg, tb = er.ln_reduce_tree(partial[:nblk].cpu())
        assert same_bits(dg, tg) and same_bits(db, tb)
    # the same kernel instance (a partial table keeps a tall batch in the fused class) with no dropout copy wanted: the same dx
    again = None if partial is None else torch.empty_like(partial)
    plain = ops.layernorm_bwd_ex(*dev, partial=again, **kw)
    assert plain["dx_drop"] is None and same_bits(plain["dx"], r["dx"])
    # p = 0 with the copy wanted: the copy is dx
    copy = ops.layernorm_bwd_ex(*dev, want_drop=True, partial=again, **kw)
    assert same_bits(copy["dx_drop"], copy["dx"]) and same_bits(copy["dx"], r["dx"])
    if partial is not None:
        assert same_bits(again[:nblk], partial[:nblk])
    # planes only: no fp32 dropout copy, its planes (and dx's) are the split of the fp32 results above
    pl = ops.layernorm_bwd_ex(*dev, drop_p=P_DROP, drop_site=site, rng=rng, partial=again, want_planes=True, want_drop_planes=True, **kw)
    assert pl["dx_drop"] is None and same_bits(pl["dx"], r["dx"])
    assert planes_are_the_split_of(pl["planes"], r["dx"]) and planes_are_the_split_of(pl["drop_planes"], r["dx_drop"])


@pytest.mark.parametrize("rows,full_rows,E", er.LN_SHORT_CASES)
def test_layernorm_bwd_short_last_batch_writes_zero_chunks(ops, rows, full_rows, E):
    x, g, b, dy, _ = er.ln_inputs(rows, E, seed=20)
    ref = er.layernorm_ref(x, g, b, dy=dy)
    nblk, live = -(-full_rows // 16), -(-rows // 16)
    partial = torch.full((nblk + 2, 2, E), math.nan, device="cuda")
    r = ops.layernorm_bwd_ex(dy.cuda(), x.cuda(), g.cuda(), _stats(ref).cuda(), partial=partial, full_rows=full_rows)
    fam = "layernorm_bwd_short_batch"
    assert r["nblk"] == nblk and all_nan(partial[nblk:])
    assert same_bits(partial[live:nblk], torch.zeros(nblk - live, 2, E))          # every chunk past the last row: exactly zero
    held(fam, "dx", r["dx"], ref["dx"], er.TOL_LN_BWD)
    held(fam, "partial", partial[:nblk], er.ln_partial_ref(dy, ref["xhat"], rows, full_rows), er.TOL_LN_BWD)
    dg, db = _reduce(ops, partial, nblk, E)
    held(fam, "dgamma", dg, ref["dgamma"], er.TOL_LN_BWD)
    held(fam, "dbeta", db, ref["dbeta"], er.TOL_LN_BWD)


def test_layernorm_zero_variance_rows_in_a_random_batch(ops):
    rows, E = er.LN_ZERO_VAR
    x, g, b, dy, _ = er.ln_inputs(rows, E, const_rows=(0, 17, rows - 1))
    ref = er.layernorm_ref(x, g, b, dy=dy)
    y, stats, _ = ops.layernorm_fwd_ex(x.cuda(), g.cuda(), b.cuda())
    fam = "layernorm_zero_variance"
    held(fam, "y", y, ref["y"], er.TOL_LN_FWD)
    held(fam, "rstd", stats[:, 1], ref["rstd"], er.TOL_STATS)
    partial = torch.full((4, 2, E), math.nan, device="cuda")
    r = ops.layernorm_bwd_ex(dy.cuda(), x.cuda(), g.cuda(), stats, partial=partial)
    held(fam, "dx", r["dx"], ref["dx"], er.TOL_LN_BWD)
    dg, db = _reduce(ops, partial, r["nblk"], E)
    held(fam, "dgamma", dg, ref["dgamma"], er.TOL_LN_BWD)
    held(fam, "dbeta", db, ref["dbeta"], er.TOL_LN_BWD)


# ==================================================================================================== ln_param_partial, by table
@pytest.fixture(scope="module")
def ln_table():
    """Six LayerNorms alternating encoder (96 rows) / decoder (6 rows) at E = 128: inputs, fp64 xhat, device copies."""
    E = er.LN_TABLE_E
    out = []
    for i in range(er.LN_TABLE_N):
        dec = i % 2
        rows = er.LN_TABLE_DEC if dec else er.LN_TABLE_ENC
        x, g, b, dy, _ = er.ln_inputs(rows, E, seed=10 * i)
        ref = er.layernorm_ref(x, g, b)
        out.append(dict(dec=dec, dy_host=dy, xhat=ref["xhat"], dy=dy.cuda(), x=x.cuda(), stats=_stats(ref).cuda()))
    return out


@pytest.mark.parametrize("rows_enc,full_enc", [(er.LN_TABLE_ENC, er.LN_TABLE_ENC)] + [(r, er.LN_TABLE_ENC) for r in er.LN_TABLE_SHORT_ENC]
                         + [(er.LN_TABLE_ENC, er.LN_TABLE_FUSED_FULL)])
def test_ln_param_partial_by_table(ops, ln_table, rows_enc, full_enc):
    """Mixed encoder / decoder entries on a grid sized by the larger class: every chunk against fp64, zero chunks past an entry's
    last row, nothing written past an entry's chunk count -- and encoder entries left alone when their class sums in the row kernel."""
    E, cap = er.LN_TABLE_E, 8
    fused = full_enc >= 1024
    entries = [dict(e, partial=torch.full((cap, 2, E), math.nan, device="cuda")) for e in ln_table]
    ops.ln_param_partial(entries, E=E, rows_enc=rows_enc, rows_dec=er.LN_TABLE_DEC, full_rows_enc=full_enc, full_rows_dec=er.LN_TABLE_DEC)
    for i, e in enumerate(entries):
        rows, full = (er.LN_TABLE_DEC, er.LN_TABLE_DEC) if e["dec"] else (rows_enc, full_enc)
        n = 0 if (fused and not e["dec"]) else -(-full // 16)
        assert n <= cap and all_nan(e["partial"][n:]), (i, n)
        if n:
            want = er.ln_partial_ref(e["dy_host"], e["xhat"], rows, full)
            for j in range(n):
                held("ln_param_partial", "dgamma_chunk", e["partial"][j, 0], want[j, 0], er.TOL_LN_BWD)
                held("ln_param_partial", "dbeta_chunk", e["partial"][j, 1], want[j, 1], er.TOL_LN_BWD)


def test_ln_param_reduce_every_loop_shape_in_one_launch(ops):
    """nblk from 1 to 1024 around the unrolled loop's trip sizes (32 per trip of four groups), E from 4 to 1024 in one launch with
    max_E = 1024: the documented order bit for bit, fp64 to 5e-5, nothing written past an entry's E."""
    pad, sentinel = 8, -7.0
    entries = []
    for i, nblk in enumerate(er.REDUCE_NBLK):
        E = er.REDUCE_E[i % len(er.REDUCE_E)]
        part = er.rnd(nblk, 2, E, seed=30 + i)
        entries.append(dict(host=part, partial=part.cuda(), nblk=nblk, E=E, dgamma=torch.full((E + pad,), sentinel, device="cuda"),
                            dbeta=torch.full((E + pad,), sentinel, device="cuda")))
    ops.ln_param_reduce(entries, max(er.REDUCE_E))
    for e in entries:
        E = e["E"]
        tg, tb = er.ln_reduce_tree(e["host"])
        assert same_bits(e["dgamma"][:E], tg) and same_bits(e["dbeta"][:E], tb), (e["nblk"], E)
        assert bool((e["dgamma"][E:] == sentinel).all()) and bool((e["dbeta"][E:] == sentinel).all())
        held("ln_param_reduce", "dgamma", e["dgamma"][:E], e["host"][:, 0].double().sum(0), er.TOL_LN_BWD)
        held("ln_param_reduce", "dbeta", e["dbeta"][:E], e["host"][:, 1].double().sum(0), er.TOL_LN_BWD)


# ========================================================================================================================= loss
def _criterion(ops, general, logits, y, ign, V):
    """The criterion on a padded logits matrix (ld = V + 5), its gradient into a padded, NaN-filled one."""
    B = logits.shape[0]
    wide = torch.full((B, V + er.LOSS_PAD), 1e30, device="cuda")
    wide[:, :V] = logits.cuda()
    dwide = torch.full((B, V + er.LOSS_PAD), math.nan, device="cuda")
    if general:
        w = er.loss_weight(V)
        got = ops.lsm_nll_ex(wide[:, :V], y.cuda(), ign, weight=w.cuda(), label_smoothing=0.1, dlogits=dwide[:, :V])
        ref = er.lsm_nll_ref(logits, y, ign, weight=w, label_smoothing=0.1)
    else:
        got = ops.lsm_nll(wide[:, :V], y.cuda(), ign, dlogits=dwide[:, :V])
        ref = er.lsm_nll_ref(logits, y, ign)
    assert all_nan(dwide[:, V:])                         # nothing written past V in a row of ld_dlogits > V
    return got, ref


def _loss_checks(fam, got, ref, y, ign, V):
    (logp, loss, dl), (r_logp, r_loss, r_dl) = got, ref
    held(fam, "logp", logp, r_logp, er.TOL_LOGP)
    held(fam, "dlogits", dl, r_dl, er.TOL_LOSS_GRAD)
    e = abs(float(loss) - float(r_loss))
    print(f"{fam} loss: {float(loss)!r} (reference {float(r_loss)!r})")
    assert e <= 1e-6 * abs(float(r_loss))
    ignored = ~((y != ign) & (y >= 0) & (y < V))
    if ignored.any():                                    # exactly zero, whatever the bound above would admit
        assert exactly_zero(dl.cpu()[ignored])


@pytest.mark.parametrize("general", [False, True], ids=["plain", "smoothed-weighted"])
@pytest.mark.parametrize("B,V", er.LOSS_CASES)
def test_loss_shapes(ops, B, V, general):
    logits, y, ign = er.loss_inputs(B, V)
    got, ref = _criterion(ops, general, logits, y, ign, V)
    _loss_checks("loss_general" if general else "loss", got, ref, y, ign, V)


@pytest.mark.parametrize("general", [False, True], ids=["plain", "smoothed-weighted"])
def test_loss_saturated_logits(ops, general):
    B, V = er.LOSS_SATURATED
    logits, y, ign = er.loss_inputs(B, V, scale=30.0)
    got, ref = _criterion(ops, general, logits, y, ign, V)
    _loss_checks("loss_saturated", got, ref, y, ign, V)


@pytest.mark.parametrize("general", [False, True], ids=["plain", "smoothed-weighted"])
def test_loss_every_target_ignored(ops, general):
    B, V = er.LOSS_ALL_IGNORED
    logits, y, ign = er.loss_inputs(B, V, kind="all_ignored")
    (logp, loss, dl), (r_logp, r_loss, _) = _criterion(ops, general, logits, y, ign, V)
    assert math.isnan(float(loss)) and math.isnan(float(r_loss))                  # 0 / 0, as torch
    assert exactly_zero(dl)
    held("loss", "logp", logp, r_logp, er.TOL_LOGP)


@pytest.mark.parametrize("general", [False, True], ids=["plain", "smoothed-weighted"])
def test_loss_targets_outside_the_classes_count_as_ignored(ops, general):
    B, V = er.LOSS_OOR
    logits, y, ign = er.loss_inputs(B, V, kind="oor")
    assert int(y[0]) == -3 and int(y[B - 1]) == V + 1
    got, ref = _criterion(ops, general, logits, y, ign, V)
    _loss_checks("loss_general" if general else "loss", got, ref, y, ign, V)
    assert exactly_zero(got[2][0]) and exactly_zero(got[2][B - 1])


@pytest.mark.parametrize("B,V", er.LSM_BWD_CASES)
def test_lsm_bwd_shapes(ops, B, V):
    logits, _, _ = er.loss_inputs(B, V)
    logp = torch.log_softmax(logits.double(), -1)
    dlogp = er.rnd(B, V, seed=5)
    want = dlogp.double() - torch.exp(logp) * dlogp.double().sum(1, keepdim=True)
    dwide = torch.full((B, V + er.LOSS_PAD), math.nan, device="cuda")
    got = ops.lsm_bwd(logp.float().cuda(), dlogp.cuda(), dlogits=dwide[:, :V])
    assert all_nan(dwide[:, V:])
    held("lsm_bwd", "dlogits", got, want, er.TOL_LOSS_GRAD)


# =============================================================================================================== optimizer step
def _arenas(n):
    return er.rnd(n, seed=1), er.rnd(n, seed=2, scale=1e-3), er.rnd(n, seed=3, scale=1e-3)


def _norm_held(norm, g):
    total = float(torch.sqrt((g.double() ** 2).sum()))
    e = abs(float(norm) - total) / total
    print(f"optimizer norm: {e:.2e} (bound 1.0e-05)")
    MEASURED.setdefault("optimizer", {})["norm"] = max(MEASURED.get("optimizer", {}).get("norm", 0.0), e)
    BOUNDS.setdefault("optimizer", {})["norm"] = 1e-5
    assert e < 1e-5


@pytest.mark.parametrize("n", er.OPT_N)
def test_clip_sgd_step_sizes(ops, n):
    """n = 4: one of the 1024 sum-of-squares workgroups has an element, the rest must write their zero (the partials start as
    NaN); n = 2^21 + 1024: the update's grid-stride trip."""
    from oracle import train_ref
    from slnlp import _lib
    p0, g, buf0 = _arenas(n)
    for max_norm in (0.5, 1e9):
        P, G, Bf = p0.cuda(), g.cuda(), buf0.cuda()
        lr, rng = torch.tensor([0.01], device="cuda"), ops.make_rng(1, 41)
        partials, norm = torch.full((1024,), math.nan, device="cuda"), torch.full((1,), math.nan, device="cuda")
        _lib.check(_lib.load().slnlp_clip_sgd_step(P.data_ptr(), G.data_ptr(), Bf.data_ptr(), n, lr.data_ptr(), 0.9, max_norm,
                                                   partials.data_ptr(), norm.data_ptr(), rng.data_ptr(), _lib.stream_ptr()), "clip_sgd_step")
        assert not bool(torch.isnan(partials).any())
        gg = [g.clone()]
        train_ref.clip_grad_norm(gg, max_norm)
        params, bufs = {"w": p0.clone()}, {"w": buf0.clone()}
        train_ref.sgd_momentum_step(params, {"w": gg[0]}, bufs, 0.01, 0.9)
        _norm_held(norm, g)
        held("optimizer", "sgd_params", P, params["w"], 1e-6)
        held("optimizer", "sgd_momentum", Bf, bufs["w"], 1e-6)
        assert int(rng[1]) == 42


@pytest.mark.parametrize("n", er.OPT_N)
def test_clip_sgd_step_ex_sizes(ops, n):
    from oracle import train_ref
    p0 = er.rnd(n, seed=1)
    P, Bf, cnt = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(1, device="cuda")
    lr = torch.tensor([0.05], device="cuda")
    ref = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.SGD([ref], lr=0.05, momentum=0.9, weight_decay=1e-2)
    for step in range(2):
        g = er.rnd(n, seed=20 + step, scale=1e-2 if step % 2 else 1e-4)
        norm = ops.clip_sgd_step_ex(P, g.cuda(), Bf, lr, cnt, momentum=0.9, max_norm=0.5, weight_decay=1e-2)
        gg = [g.clone().double()]
        train_ref.clip_grad_norm(gg, 0.5)
        ref.grad = gg[0]
        opt.step()
        _norm_held(norm, g)
        held("optimizer", "sgd_ex_params", P, ref, 1e-6)
        held("optimizer", "sgd_ex_momentum", Bf, opt.state[ref]["momentum_buffer"], 1e-5)
    assert float(cnt) == 2.0


@pytest.mark.parametrize("n", er.OPT_N)
def test_clip_adam_step_sizes(ops, n):
    p0 = er.rnd(n, seed=1)
    P, M1, M2 = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    lr, cnt = torch.tensor([3e-3], device="cuda"), torch.zeros(1, device="cuda")
    ref = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.Adam([ref], lr=3e-3, betas=(0.9, 0.99), eps=1e-8)
    for step in range(2):
        g = er.rnd(n, seed=10 + step, scale=1e-2 if step % 2 else 1e-4)
        norm = ops.clip_adam_step(P, g.cuda(), M1, M2, lr, cnt, betas=(0.9, 0.99), eps=1e-8, max_norm=0.5)
        ref.grad = g.clone().double()
        torch.nn.utils.clip_grad_norm_([ref], 0.5)
        opt.step()
        _norm_held(norm, g)
        worst = float((P.cpu().double() - ref.detach()).abs().max())
        print(f"optimizer adam_params: {worst:.2e} absolute (bound {1e-6 * (step + 1):.1e})")
        assert worst < 1e-6 * (step + 1), step              # |w| < 8: one fp32 ulp (9.5e-7) per step
    assert float(cnt) == 2.0
    st = opt.state[ref]
    held("optimizer", "adam_exp_avg", M1, st["exp_avg"], 1e-5)
    held("optimizer", "adam_exp_avg_sq", M2, st["exp_avg_sq"], 1e-5)
