"""CPU: tests/attention_ref.py is torch's multi-head attention, its error measure sees one wrong block, and every case of the GPU
edge tests (tests/test_attn_edges_gpu.py) meets the conditions its bounds rest on."""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_ref as ar
import kernel_refs as kr


@pytest.mark.parametrize("B,S,H,dh", [(3, 17, 2, 8), (2, 19, 1, 192)])
def test_reference_is_torch_multi_head_attention(B, S, H, dh):
    """Identity projections, causal mask plus key padding mask, dropout 0, per-head weights: ctx and probs of mha_ref."""
    E = H * dh
    inp = ar.self_inputs(B, S, H, dh)
    qkv = inp["qkv"].double()
    q, k, v = [qkv[:, i * E:(i + 1) * E].reshape(S, B, E) for i in range(3)]
    eye = torch.eye(E, dtype=torch.float64)
    out, w = F.multi_head_attention_forward(
        q, k, v, E, H, None, None, None, None, False, 0.0, eye, None, training=False, key_padding_mask=inp["ids"] == ar.PAD,
        need_weights=True, attn_mask=torch.triu(torch.ones(S, S, dtype=torch.bool), 1), use_separate_proj_weight=True,
        q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye, average_attn_weights=False)
    ctx, pr = ar.mha_ref(qkv, inp["ids"], ar.PAD, B, S, H, dh, True)
    assert not torch.isnan(out).any()
    assert ar.block_err(pr, w) < 1e-14
    assert ar.block_err(ctx, out.reshape(S * B, E), B, H) < 1e-14


@pytest.mark.parametrize("case", ar.SELF_EDGE, ids=ar.case_id)
def test_every_edge_case_leaves_float32_its_margin(case):
    """No NaN in the fp64 reference; torch float32 stays within COND of it per block on all three tensors, so a bound of a few
    x e_fmt is a statement about the kernel and not about the inputs; the format yardstick is where the formats put it."""
    B, S, H, dh = case
    inp = ar.self_inputs(B, S, H, dh)
    ref, e_fp32, e_fmt = ar.attn_yardsticks(inp, B, S, H, dh)
    print(case, {k: f"{v:.2e}" for k, v in e_fp32.items()}, {k: f"{v:.2e}" for k, v in e_fmt.items()})
    for k in ("probs", "ctx", "dqkv"):
        assert not torch.isnan(ref[k]).any(), k
        assert e_fp32[k] <= ar.COND, (k, e_fp32[k])
        assert e_fmt[k] < 1e-4, (k, e_fmt[k])                  # three bf16 passes: ~2^-16 per product, never bf16's own 2^-9
    if S == 1:
        assert e_fmt["probs"] == 0.0                           # softmax of one element


def test_cases_are_the_edges_the_kernels_branch_on():
    """The table holds what the GPU file relies on: every shape is one the launchers accept, at most 64 x 64 x 256 per head
    and 12 blocks, and each named edge is present."""
    for B, S, H, dh in ar.SELF_EDGE:
        assert 1 <= S <= 64 and dh % 4 == 0 and dh <= 256 and (dh <= 64 or dh % 64 == 0) and B * H <= 12
    S_set, dh_set = {c[1] for c in ar.SELF_EDGE}, {c[3] for c in ar.SELF_EDGE}
    assert {1, 16, 17, 32, 33, 63, 64} <= S_set and {4, 12, 24, 40, 64, 128, 192, 256} <= dh_set
    assert any(c[0] == 1 for c in ar.SELF_EDGE) and any(c[2] == 1 for c in ar.SELF_EDGE)
    assert all(S > 64 for _, S, _, _ in ar.LONG_PLANES)
    for shape, _, _ in ar.SELF_VARIANTS:
        assert shape in ar.SELF_EDGE


def test_block_err_sees_one_small_block_and_lost_planes():
    """What the per-block measure is for: a (batch, head) block 1000 x smaller than the rest, wrong by 1e-3 of itself, is 1e-6
    of the tensor maximum and 1e-3 per block; a NaN or a nonzero value against an all-zero block is an infinite error."""
    B, S, H, dh = 2, 5, 2, 4
    ref = ar.rnd(S * B, H * dh, seed=4).double()
    blocks = ref.view(S, B, H, dh)
    blocks[:, 1, 0] *= 1e-3
    got = ref.clone()
    got.view(S, B, H, dh)[:, 1, 0] *= 1 + 1e-3
    assert kr.rel(got, ref) < 2e-6 and 5e-4 < ar.block_err(got, ref, B, H) <= 1e-3
    bad = ref.clone()
    bad[3, 2] = math.nan
    assert ar.block_err(bad, ref, B, H) == math.inf
    zero = ref.clone()
    zero.view(S, B, H, dh)[:, 0, 1] = 0
    assert ar.block_err(zero, zero, B, H) == 0.0 and ar.block_err(ref, zero, B, H) == math.inf
    # dqkv: the head's three column groups are one block
    g = ar.rnd(S * B, 3 * H * dh, seed=5).double()
    g2 = g.clone()
    g2.view(S, B, 3, H, dh)[0, 1, 2, 1, 0] += 1.0
    assert ar.block_err(g2, g, B, H, parts=3) > 0.1
    # a lost lo plane is 2^-9, inside no format bound; hi + lo is 2^-16
    x = ar.rnd(S * B, H * dh, seed=6)
    hi, lo = kr.bf16_split(x)
    assert ar.block_err(hi, x, B, H) > ar.bound(1.4e-5, ar.COND) > ar.block_err(hi + lo, x, B, H)


def test_format_product_rounds_both_gradient_products():
    """fmt_product(3) is fmt_matmul in the forward and in both of autograd's products."""
    a = ar.rnd(2, 3, 5, 7, seed=1).double().requires_grad_(True)
    b = ar.rnd(2, 3, 7, 4, seed=2).double().requires_grad_(True)
    g = ar.rnd(2, 3, 5, 4, seed=3).double()
    out = ar.fmt_product(3)(a, b)
    out.backward(g)
    assert torch.equal(out.detach(), kr.fmt_matmul(a.detach(), b.detach(), 3))
    assert torch.equal(a.grad, kr.fmt_matmul(g, b.detach().transpose(-1, -2), 3))
    assert torch.equal(b.grad, kr.fmt_matmul(a.detach().transpose(-1, -2), g, 3))
    assert 0 < kr.rel(out, a.detach() @ b.detach()) < 1e-4
