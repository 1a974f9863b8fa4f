"""GPU parity of the attention kernels for sequences beyond one 64-key tile (attention_long.hip: one wave per attention row)
through the C ABI against fp64 restatements (tests/kernel_refs.py) and fp64 autograd, up to S = 4100 where the kernels' dynamic
LDS limit is raised.  Tolerances (max|got - ref| / max|ref| per tensor, printed per case): plain fp32 FMA kernels, so the
class of exact-fp32 kernels in test_kernels_gpu.py, 2e-5; their backward tensors 5e-5, as test_attn_cross there."""
import pytest
import torch

from kernel_refs import _mha_ref, cross_ref, rel

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_BWD = 2e-5, 5e-5


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    return o


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _keep_mask(ops, rows, cols, p, site, rng):
    m = ops.dropout_mask(rows, cols, p, site, rng).cpu()
    assert 0 < float(m.sum()) < m.numel()                                  # kept and dropped elements
    return m.double()


def _self_case(ops, B, S, H, dh, p, causal=True, use_ids=True):
    E = H * dh
    qkv = rnd(S * B, 3 * E, seed=1).double().requires_grad_(True)
    ids = None
    if use_ids:
        lengths = torch.randint(max(1, S // 6), S + 1, (B,), generator=torch.Generator().manual_seed(3))
        lengths[0] = S // 2
        ids = torch.full((B, S), 5, dtype=torch.long)
        ids[torch.arange(S)[None, :] >= lengths[:, None]] = 1
        assert (ids == 1).any() and not (ids == 1).all(1).any()
    rng = ops.make_rng(seed=5, step=2)
    mask = _keep_mask(ops, B * H * S, S, p, 17, rng).view(B, H, S, S) if p > 0 else None
    ctx_ref, pr_ref = _mha_ref(qkv, ids, 1, B, S, H, dh, causal, mask, p)
    dctx = rnd(S * B, E, seed=2)
    ctx_ref.backward(dctx.double())
    assert all(torch.isfinite(x).all() for x in (ctx_ref, pr_ref, qkv.grad))
    qc, idc = qkv.detach().float().cuda(), (None if ids is None else ids.cuda())
    ctx, probs = ops.attn_self_fwd(qc, idc, 1, B=B, S=S, H=H, dh=dh, causal=causal, drop_p=p, drop_site=17, rng=rng)
    dqkv = ops.attn_self_bwd(qc, probs, dctx.cuda(), B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=17, rng=rng)
    again = ops.attn_self_bwd(qc, probs, dctx.cuda(), B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=17, rng=rng)
    assert torch.equal(dqkv, again)                                        # two calls are bit-identical
    errs = dict(probs=rel(probs, pr_ref), ctx=rel(ctx, ctx_ref))
    for i, n in enumerate(("dq", "dk", "dv")):
        errs[n] = rel(dqkv[:, i * E:(i + 1) * E], qkv.grad[:, i * E:(i + 1) * E])
    print(f"attn_self_long B{B} S{S} H{H} dh{dh} p{p} causal{int(causal)} ids{int(use_ids)}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    blocked = pr_ref == 0
    assert torch.all(probs.cpu()[blocked] == 0)                            # blocked keys weigh exactly 0
    assert errs["probs"] < TOL_FWD and errs["ctx"] < TOL_FWD
    assert errs["dq"] < TOL_BWD and errs["dk"] < TOL_BWD and errs["dv"] < TOL_BWD


SELF_SHAPES = [(3, 65, 2, 8), (2, 128, 2, 128), (2, 200, 4, 32), (1, 1030, 1, 36), (2, 97, 1, 256), (1, 4100, 1, 8)]


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("B,S,H,dh", SELF_SHAPES)
def test_attn_self_long(ops, B, S, H, dh, p):
    """Causal + pad mask; head dims below one wave (36), of one to four values per lane, S = 4100 on the raised LDS limit."""
    _self_case(ops, B, S, H, dh, p)


@pytest.mark.parametrize("causal,use_ids", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("B,S,H,dh", [(3, 65, 2, 8), (2, 128, 2, 128), (2, 97, 1, 256)])
def test_attn_self_long_without_causal_mask_or_ids(ops, B, S, H, dh, p, causal, use_ids):
    """causal = 0 and ids = NULL, alone and together, at the smallest shapes."""
    _self_case(ops, B, S, H, dh, p, causal=causal, use_ids=use_ids)


def test_attn_self_long_fully_masked_row_is_nan_for_that_row_only(ops):
    # a sequence whose first key is <pad>: query 0 has no visible key -> NaN like torch (test_kernels_gpu.py asserts it at S = 8)
    B, S, H, dh = 2, 70, 2, 8
    qkv = rnd(S * B, 3 * H * dh, seed=1)
    ids = torch.full((B, S), 5, dtype=torch.long)
    ids[1, 0] = 1
    _, pr_ref = _mha_ref(qkv.double(), ids, 1, B, S, H, dh, True)
    ctx, probs = ops.attn_self_fwd(qkv.cuda(), ids.cuda(), 1, B=B, S=S, H=H, dh=dh)
    probs = probs.cpu()
    assert torch.isnan(pr_ref[1, :, 0]).all() and torch.isnan(probs[1, :, 0]).all()
    assert not torch.isnan(probs[0]).any() and not torch.isnan(probs[1, :, 1:]).any()
    assert rel(probs[0], pr_ref[0]) < TOL_FWD and rel(probs[1, :, 1:], pr_ref[1, :, 1:]) < TOL_FWD


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("B,S,H,dh", [(4, 65, 2, 8), (3, 300, 4, 64), (2, 2048, 2, 256), (1, 4100, 1, 8)])
def test_attn_cross_long(ops, B, S, H, dh, p):
    """One query per sequence over S memory rows; kv and dkv live in wider buffers (row strides 2E + 8 and 2E + 12) whose pad
    columns hold NaN (kv) and a sentinel that must survive (dkv)."""
    E = H * dh
    q = rnd(B, E, seed=1).double().requires_grad_(True)
    kv = rnd(S * B, 2 * E, seed=2).double().requires_grad_(True)
    rng = ops.make_rng(seed=8, step=1)
    mask = _keep_mask(ops, B * H, S, p, 9, rng).view(B, H, S) if p > 0 else None
    ctx_ref, pr_ref = cross_ref(q, kv, B, S, H, dh, mask, p)
    dctx = rnd(B, E, seed=3)
    ctx_ref.backward(dctx.double())
    assert all(torch.isfinite(x).all() for x in (ctx_ref, pr_ref, q.grad, kv.grad))
    kv_wide = torch.full((S * B, 2 * E + 8), float("nan")).cuda()
    kv_wide[:, :2 * E] = kv.detach().float().cuda()
    dkv_wide = torch.full((S * B, 2 * E + 12), 3.0).cuda()
    qc, kvc, dkv = q.detach().float().cuda(), kv_wide[:, :2 * E], dkv_wide[:, :2 * E]
    ctx, probs = ops.attn_cross_fwd(qc, kvc, B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=9, rng=rng)
    dq, _ = ops.attn_cross_bwd(qc, kvc, probs, dctx.cuda(), B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=9, rng=rng, dkv=dkv)
    dq2, dkv2 = ops.attn_cross_bwd(qc, kvc, probs, dctx.cuda(), B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=9, rng=rng)
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)                 # two calls are bit-identical
    assert torch.all(dkv_wide[:, 2 * E:] == 3.0)                           # the pad columns stay as pre-filled
    errs = dict(probs=rel(probs, pr_ref), ctx=rel(ctx, ctx_ref), dq=rel(dq, q.grad), dk=rel(dkv[:, :E], kv.grad[:, :E]),
                dv=rel(dkv[:, E:], kv.grad[:, E:]))
    print(f"attn_cross_long B{B} S{S} H{H} dh{dh} p{p}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert errs["probs"] < TOL_FWD and errs["ctx"] < TOL_FWD
    assert errs["dq"] < TOL_BWD and errs["dk"] < TOL_BWD and errs["dv"] < TOL_BWD
