"""Plain reference, yardsticks and case tables for the self-attention kernels of csrc/attention.hip as the plans call them
(tests/test_attn_edges_gpu.py runs the cases, tests/test_attention_ref_cpu.py judges the reference and the conditions the GPU
bounds rest on).  Everything is torch on the CPU; no device anywhere in this file.

The rule for the fp32 outputs is the one of tests/test_rnn_kernels_gpu.py: per tensor and case, bound = 4 x (e_fmt + e_fp32)
floored at 2e-5, where e_fp32 is the same formula in torch float32 and e_fmt the fp64 formula whose products run on
format-rounded operands (kernel_refs.fmt_matmul, precision 3: the three MFMA passes of the split-bf16 tiles).  Errors are
measured per (batch, head) block against the block's own maximum (block_err): one max over the whole tensor hides a block
that is wrong at small magnitude."""
import math

import torch

import kernel_refs as kr

PAD, REAL = 1, 5            # the pad id and the id of every real token
DROP_SITE = 17
CHAIN_FACTOR, TOL_FP32 = 4.0, 2e-5          # tests/test_rnn_kernels_gpu.py
COND = 2e-6                 # torch float32 against fp64 on a case's inputs: the inputs must leave fp32 this margin

# (B, S, H, dh): the edges of the one-tile kernels (64 x 64 keys, head dim in 64-wide chunks, four waves of 16 rows)
SELF_EDGE = [
    (2, 1, 2, 8),                                        # one key: softmax of one element, three idle waves
    (3, 16, 2, 8), (3, 17, 2, 8),                        # last row of wave 0 / first row of wave 1
    (2, 32, 1, 16), (2, 33, 1, 16),                      # one K step over the keys vs. two; H = 1
    (2, 63, 2, 8),                                       # one row and one column short of the tile
    (1, 64, 2, 64),                                      # B = 1, full tile, full chunk
    (3, 20, 4, 4), (3, 20, 2, 12),                       # dh % 8 != 0: element stores with the fp32 output NULL
    (3, 20, 2, 24), (2, 37, 2, 40),                      # row pieces cut inside a 64-wide row; a partly filled 16-column piece
    (2, 37, 1, 128), (2, 19, 1, 192), (1, 64, 1, 256),   # 2, 3 and 4 chunks: separate dS tile, row pieces through the dO tile
]
# (causal, ids) other than (True, True), at these two shapes
SELF_VARIANTS = [(shape, c, i) for shape in [(3, 17, 2, 8), (2, 19, 1, 192)] for c, i in [(False, True), (True, False), (False, False)]]
LONG_PLANES = [(3, 65, 2, 8), (2, 97, 1, 128)]           # the wave-per-row kernels: fp32 and planes together
CROSS_PLANES = [(4, 12, 4, 8), (3, 64, 2, 64), (2, 37, 1, 128), (4, 65, 2, 8)]
CROSS_LD_PAD = 8                                         # ld_kv = ld_dkv = 2E + 8: the stride is not the width


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def case_id(case):
    return "-".join(str(int(v)) for v in case)


# ------------------------------------------------------------------------------------------------ the restatement
class _FmtBmm(torch.autograd.Function):
    """a @ b (batched) whose forward and both backward products run through kernel_refs.fmt_matmul."""

    @staticmethod
    def forward(ctx, a, b, precision):
        ctx.save_for_backward(a, b)
        ctx.precision = precision
        return kr.fmt_matmul(a, b, precision)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return kr.fmt_matmul(g, b.transpose(-1, -2), ctx.precision), kr.fmt_matmul(a.transpose(-1, -2), g, ctx.precision), None


def fmt_product(precision=3):
    """product(a, b) = a @ b on format-rounded operands, in the forward and in autograd's two products of it: with mha_ref that
    is Q K^T, P V and the four gradient contractions dP = dO V^T, dV = Pd^T dO, dQ = dS K, dK = dS^T Q."""
    return lambda a, b: _FmtBmm.apply(a, b, precision)


mha_ref = kr._mha_ref       # the restatement (kernel_refs.py: shared with the long-sequence tests), its product exposed


# ------------------------------------------------------------------------------------------------ inputs
def self_inputs(B, S, H, dh, use_ids=True):
    """The inputs of test_kernels_gpu.py::test_attn_self: seeded normal qkv and d ctx (float32 values), lengths from
    randint(max(1, S // 6), S + 1) with the padding at the tail, so no query row is fully masked under the causal mask."""
    E = H * dh
    qkv, dctx = rnd(S * B, 3 * E, seed=1), rnd(S * B, E, seed=2)
    lengths = torch.randint(max(1, S // 6), S + 1, (B,), generator=torch.Generator().manual_seed(3))
    ids = torch.full((B, S), REAL, dtype=torch.long)
    ids[torch.arange(S)[None, :] >= lengths[:, None]] = PAD
    return dict(qkv=qkv, dctx=dctx, ids=ids if use_ids else None, lengths=lengths)


def cross_inputs(B, S, H, dh):
    """q [B, E], kv [S*B, 2E] as a column view of a [S*B, 2E + CROSS_LD_PAD] buffer, d ctx [B, E]."""
    E = H * dh
    wide = rnd(S * B, 2 * E + CROSS_LD_PAD, seed=2)
    return dict(q=rnd(B, E, seed=1), kv_wide=wide, kv=wide[:, :2 * E], dctx=rnd(B, E, seed=3))


# ------------------------------------------------------------------------------------------------ errors and yardsticks
def block_err(got, ref, B=None, H=None, parts=1):
    """The error per (batch, head) block: max |got - ref| over the block / that block's own max |ref|, the worst block.
    4-D tensors ([B, H, S, S] probs) take their two leading dims; 2-D ones ([S*B, parts * E], rows time-major) need B and H, and a
    block is the head's dh-wide column group in each of the ``parts`` (3 for dqkv: its dQ, dK and dV columns together).
    A NaN against a number, or anything but zero against an all-zero block, is an infinite error."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.ndim == 4:
        d = (got - ref).abs().flatten(2)
        r = ref.abs().flatten(2)
    else:
        rows, W = ref.shape
        S, dh = rows // B, W // (parts * H)
        assert S * B == rows and parts * H * dh == W
        blocks = lambda t: t.view(S, B, parts, H, dh).permute(1, 3, 0, 2, 4).reshape(B, H, -1)
        d, r = blocks((got - ref).abs()), blocks(ref.abs())
    d, top = d.max(-1).values, r.max(-1).values
    e = torch.where(top > 0, d / top.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    return float(e.max())


def bound(e_fmt, e_fp32):
    return max(CHAIN_FACTOR * (e_fmt + e_fp32), TOL_FP32)


def attn_eval(inp, B, S, H, dh, causal=True, mask=None, p=0.0, dtype=torch.float64, product=torch.matmul):
    """Forward of mha_ref and autograd's backward of sum(dctx * ctx) in ``dtype`` -> dict of float64 probs, ctx, dqkv."""
    qkv = inp["qkv"].detach().to(dtype).clone().requires_grad_(True)
    ctx, pr = mha_ref(qkv, inp["ids"], PAD, B, S, H, dh, causal, None if mask is None else mask.to(dtype), p, product)
    ctx.backward(inp["dctx"].to(dtype))
    return dict(probs=pr.detach().double(), ctx=ctx.detach().double(), dqkv=qkv.grad.double())


def errors(got, ref, B, H):
    """block_err of probs, ctx and dqkv (those of them ``got`` holds)."""
    parts = dict(probs=1, ctx=1, dqkv=3)
    return {k: block_err(got[k], ref[k], B, H, parts[k]) for k in parts if k in got}


def attn_yardsticks(inp, B, S, H, dh, causal=True, mask=None, p=0.0, precision=3):
    """-> (ref, e_fp32, e_fmt) for probs, ctx and dqkv, in the manner of kernel_refs.chain_yardsticks: the fp64 reference, and
    the block_err against it of the same formula in torch float32 and of the fp64 formula with format-rounded products."""
    ref = attn_eval(inp, B, S, H, dh, causal, mask, p)
    f32 = attn_eval(inp, B, S, H, dh, causal, mask, p, dtype=torch.float32)
    fmt = attn_eval(inp, B, S, H, dh, causal, mask, p, product=fmt_product(precision))
    return ref, errors(f32, ref, B, H), errors(fmt, ref, B, H)


# ------------------------------------------------------------------------------------------------ planes
def planes_value(planes):
    """hi + lo of int16 bf16 bit patterns, float64."""
    hi, lo = [t.detach().cpu().contiguous().view(torch.bfloat16).double() for t in planes]
    return hi + lo
