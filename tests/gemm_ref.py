"""Cases, references and yardsticks for the three GEMM families -- csrc/gemm.hip (fp32 operands, split on the way into LDS),
csrc/gemm_planes.hip (pre-split bf16 hi / lo planes) and csrc/gemm_rows.hip (the decoder's B-row products) --
tests/test_gemm_edges_gpu.py runs the cases, tests/test_gemm_ref_cpu.py judges what is in here.  Everything is torch on the
CPU; no device anywhere in this file.

Two kinds of case.

INTEGER cases: the kernels must be exact, so they are held bit for bit.  A bf16 product of two integers is exact and an fp32 sum
of integers is exact while it stays below 2^24, so on suitable integer operands every MFMA pass, every partial tile, every
split-K partial and the whole epilogue are exact: one right answer whatever the accumulation order.  "Tailed" operands mix
+- odd integers in [257, 511] -- nine significant bits, so hi and lo are both non-zero and hi + lo is the value -- with integers
in [-4, 4]; "short" operands hold integers in [-4, 4] only (their lo plane is zero).  Precision p then has ONE expected value,

    3:  A B^T - A_lo B_lo^T      2:  A_hi (B_hi + B_lo)^T      1:  A_hi B_hi^T

and rowsum_a is the sum over k of the A planes the product reads (hi + lo at precision 3 -- plane_kloop's `if (NPA == 2) t +=`,
rows_wgrad_unit's `la` x ones, TileIO::value<3> -- hi alone at 1 and 2).  The three differ on every case, so the test also
says WHICH passes ran.  The condition is SUM_LIMIT: max over (m, n) of sum_k |a||b| < 2^22, two spare bits under fp32's 24.

FLOAT cases: unit Gaussians times a power of two per row (2^-12 .. 2^12, A and B independently), judged componentwise,

    err = max over (m, n) of |got - ref| / (|A| |B|^T + |bias| + |resid|)[m, n]

so that a wrong element in a small row counts as much as one in a large row, against bound = 4 x (e_fmt + e_fp32) floored at
2e-5 (the rule of tests/test_rnn_kernels_gpu.py and tests/test_attn_edges_gpu.py): e_fmt the same error of the fp64 product
of format-rounded operands, e_fp32 that of a float32 product summed per 64-k tile in tile order.

The fp32-operand family splits differently from the other two at precision 3: its hi is the TRUNCATED upper half of the fp32
word and lo = bf16(x - hi) (mfma_tile.hpp, stash) where the planes and gemm_rows round hi to nearest (split_bf16).  hi + lo is
the value either way on these integers, but A_lo B_lo^T differs, and on floats the truncated split leaves up to 2^-14 per product
where the rounded one leaves 2^-16: `split_of(family)` says which one a family's expected values and e_fmt are made with."""
import math

import torch

import kernel_refs as kr

SUM_LIMIT = 2 ** 22                     # the integer cases' condition on max sum_k |a||b|
EXACT_LIMIT = 2 ** 24                   # ... and on every value an epilogue of theirs passes through
TAIL_SHARE, TT_SHARE = 0.6, 0.25        # share of tailed elements drawn: one tailed operand / both (K <= 64 only)
TAIL_FLOOR = {TAIL_SHARE: 0.40, TT_SHARE: 0.125}     # at least this share of a tailed operand of 64 elements or more has a non-zero lo
CHAIN_FACTOR, TOL_FP32 = 4.0, 2e-5      # tests/test_rnn_kernels_gpu.py
COND = 2e-6                             # float32 against fp64 on a case's inputs (attention_ref.COND)
KT = 64                                 # the K tile of every family
DROP_P, GATE_SCALE = 0.5, 2.0           # an exact epilogue: 1 / (1 - p) = 2

LAYOUTS = ("forward", "dgrad", "wgrad")
PAIRINGS = ("TS", "ST")                 # (A, B) kinds; "TT" where tt_applies
# ---- the smallest shapes that reach each edge: every listed value at least once per table (test_gemm_ref_cpu.py checks), not the product
PLANE_SHAPES = [(1, 4, 4), (63, 60, 60), (64, 64, 64), (65, 68, 68), (96, 192, 132), (97, 64, 576), (130, 60, 1536)]      # (M, N, K)
PLANE_KNOBS = (64, 96, 128, 12832, 256)
PLANE_GEO = {64: 0, 128: 1, 12832: 2, 256: 3, 96: 4}
PLANE_SPLITS = {(65, 68, 68): (2, 3, 8, 5), (97, 64, 576): (2, 3, 8, 12), (130, 60, 1536): (2, 3, 8, 27)}     # the last: more than the K tiles
PLANE_EPI_SHAPES = [(65, 68, 68), (97, 64, 576)]
# one grouped launch: four jobs, four shapes, every layout, precisions 3 and 2 sharing the launch: (layout, precision, shape, split)
PLANE_GROUP = [("forward", 3, (65, 68, 68), 1), ("dgrad", 2, (96, 192, 132), 1), ("wgrad", 2, (63, 60, 576), 3), ("wgrad", 3, (130, 60, 1536), 8)]
ROWS_SHAPES = [(1, 1, 64), (15, 15, 448), (16, 16, 512), (17, 17, 576), (50, 202, 960), (64, 16, 1024), (65, 15, 64), (130, 17, 576),
               (50, 202, 64)]
ROWS_TILES = (0, 1, 2)
ROWS_EPI_SHAPES = [(17, 17, 576), (50, 202, 64)]
ROWS_BWD_SHAPES = [(1, 64, 4), (15, 576, 12), (17, 1024, 20), (50, 64, 64), (64, 576, 132), (130, 1024, 200)]             # (B, Nout, Kin)
F32_SHAPES = [(1, 1, 1), (7, 5, 3), (65, 65, 63), (7, 1, 64), (65, 130, 65), (65, 5, 192), (1, 130, 257)]
F32_KS = (1, 2)
F32_EPI_SHAPES = [(7, 5, 3), (65, 65, 63), (65, 5, 192)]
F32_BATCH = (3, 2, 8)                   # (B, H, dh) of the batched per-head jobs (tests/test_attn_mem_gpu.py)


def case_id(case):
    return "-".join(str(v) for v in case)


def ktiles(K):
    return (K + KT - 1) // KT


def tt_applies(M, N, K):
    """Both operands tailed: only where the drawn data can meet SUM_LIMIT (511 x 511 x K does not beyond K = 16; the smaller
    share does up to one K tile), and where an operand has enough elements that a quarter of them is some."""
    return K <= KT and M * K >= 256 and N * K >= 256


def pairings(M, N, K):
    return PAIRINGS + (("TT",) if tt_applies(M, N, K) else ())


# ------------------------------------------------------------------------------------------------ operands
def int_operand(rows, cols, kind, seed, share=TAIL_SHARE):
    """Integers as float32 [rows, cols]: kind "S" = short, [-4, 4]; "T" = tailed, a ``share`` of +- odd integers in [257, 511]."""
    g = torch.Generator().manual_seed(seed)
    small = torch.randint(-4, 5, (rows, cols), generator=g)
    # no zero in the last row and column: whichever of the two is the last k of a product, the element a K loop is most likely
    # to lose, it always contributes
    small[-1] = torch.where(small[-1] == 0, torch.ones_like(small[-1]), small[-1])
    small[:, -1] = torch.where(small[:, -1] == 0, torch.ones_like(small[:, -1]), small[:, -1])
    if kind == "S":
        return small.float()
    big = (2 * torch.randint(128, 256, (rows, cols), generator=g) + 1) * (2 * torch.randint(0, 2, (rows, cols), generator=g) - 1)
    pick = torch.rand(rows, cols, generator=g) < share
    return torch.where(pick, big, small).float()


def int_pair(M, N, K, pairing, seed=0):
    """(A [M, K], B [N, K]) of the pairing "TS" / "ST" / "TT"."""
    share = TT_SHARE if pairing == "TT" else TAIL_SHARE
    return int_operand(M, K, pairing[0], 11 + seed, share), int_operand(N, K, pairing[1], 23 + seed, share)


def int_vector(n, seed, lo=-64, hi=65):
    return torch.randint(lo, hi, (n,), generator=torch.Generator().manual_seed(seed)).float()


def int_matrix(rows, cols, seed, lo=-64, hi=65):
    return torch.randint(lo, hi, (rows, cols), generator=torch.Generator().manual_seed(seed)).float()


def float_operand(rows, cols, seed):
    """Unit Gaussians times a power of two per row, 2^-12 .. 2^12."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    e = torch.randint(-12, 13, (rows, 1), generator=g)
    return (x * torch.pow(2.0, e.double()).float()).float()


def float_pair(M, N, K, seed=0):
    return float_operand(M, K, 31 + seed), float_operand(N, K, 47 + seed)


def bwd_operands(shape, kind):
    """(dY [B, Nout], W [Nout, Kin], X [B, Kin]) of a gemm_rows_bwd case: dY is the A operand of both products, so "TS" = dY
    tailed with W and X short, "ST" = dY short with W and X tailed, "TT" all three tailed; "float" see below."""
    Bt, Nout, Kin = shape
    if kind == "float":
        # dY[b, n] = g 2^(e_b + f_n), W[n, k] = g 2^(-f_n + h_k), X[b, k] = g 2^(-e_b + i_k): the logical operands of BOTH products carry
        # a power of two per row (2^e_b, 2^h_k for dX = dY W; 2^f_n, 2^i_k for dW = dY^T X) and none along their k
        g = torch.Generator().manual_seed(61)
        e, f, h, i = [torch.randint(-6, 7, (n,), generator=g).double() for n in (Bt, Nout, Kin, Kin)]
        two = lambda r, c: torch.pow(2.0, r[:, None] + c[None, :]).float()
        return (torch.randn(Bt, Nout, generator=g) * two(e, f), torch.randn(Nout, Kin, generator=g) * two(-f, h),
                torch.randn(Bt, Kin, generator=g) * two(-e, i))
    share = TT_SHARE if kind == "TT" else TAIL_SHARE
    return int_operand(Bt, Nout, kind[0], 61, share), int_operand(Nout, Kin, kind[1], 62, share), int_operand(Bt, Kin, kind[1], 63, share)


FAMILIES = {"planes": PLANE_SHAPES, "rows": ROWS_SHAPES, "rows_bwd": ROWS_BWD_SHAPES, "fp32": F32_SHAPES}


def products(family, shape, kind):
    """The products of a case as [(output, A [M, K], B [N, K])]: one for the forward families, the data gradient dX = dY W and
    the weight gradient dW = dY^T X (whose row sums are db) for gemm_rows_bwd."""
    if family == "rows_bwd":
        dY, W, X = bwd_operands(shape, kind)
        return [("dX", dY, W.T.contiguous()), ("dW", dY.T.contiguous(), X.T.contiguous())]
    return [("C",) + (float_pair(*shape) if kind == "float" else int_pair(*shape, kind))]


def case_pairings(family, shape):
    if family == "rows_bwd":
        Bt, Nout, Kin = shape
        return PAIRINGS + (("TT",) if tt_applies(Bt, Kin, Nout) and tt_applies(Nout, Kin, Bt) else ())
    return pairings(*shape)


# ------------------------------------------------------------------------------------------------ the formats
def trunc_split(x):
    """gemm.hip's precision-3 split of a float32 tensor: hi = the upper 16 bits of the word, lo = bf16(x - hi) (x's dtype kept)."""
    f = x.float()
    hi = (f.view(torch.int32) & -65536).view(torch.float32)
    lo = (f - hi).to(torch.bfloat16).float()
    return hi.to(x.dtype), lo.to(x.dtype)


def split_of(family, precision=3):
    """The hi / lo split a family makes of its operands: rounded to nearest (split_bf16) everywhere but gemm.hip at precision 3."""
    return trunc_split if family == "fp32" and precision == 3 else kr.bf16_split


def passes(A, B, split=kr.bf16_split):
    """float64 (hi hi, hi lo, lo hi, lo lo) products A . B^T of the split operands."""
    (ah, al), (bh, bl) = [[t.double() for t in split(x.float())] for x in (A, B)]
    return ah @ bh.T, ah @ bl.T, al @ bh.T, al @ bl.T


def expected(A, B, precision, split=kr.bf16_split):
    """What precision p computes, in float64 (exact on the integer cases): 3 = all but lo lo, 2 = A's head with both planes of B,
    1 = the heads."""
    hh, hl, lh, _ = passes(A, B, split)
    return hh if precision == 1 else hh + hl if precision == 2 else hh + hl + lh


def expected_rowsum(A, precision, split=kr.bf16_split):
    """rowsum_a: sum over k of the A planes the product reads."""
    ah, al = [t.double() for t in split(A.float())]
    return (ah + al).sum(1) if precision == 3 else ah.sum(1)


def fmt_matmul(a, b, precision, split=kr.bf16_split):
    """kernel_refs.fmt_matmul with precision 2 added (the head of a times both planes of b), for a [M, K] and b [K, N], and with
    the split of the family."""
    if precision != 2 and split is kr.bf16_split:
        return kr.fmt_matmul(a, b, precision)
    (ah, al), (bh, bl) = split(a), split(b)
    return ah @ bh if precision == 1 else ah @ bh + ah @ bl if precision == 2 else ah @ bh + ah @ bl + al @ bh


def fp32_tiled(A, B):
    """A B^T in float32, one product per 64-k tile, the partial products added in tile order -> float64."""
    A, B = A.float(), B.float()
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float32)
    for k0 in range(0, A.shape[1], KT):
        acc = acc + A[:, k0:k0 + KT] @ B[:, k0:k0 + KT].T
    return acc.double()


def epilogue(prod, *, bias=None, relu=False, gate=None, gate_scale=1.0, mask=None, drop_scale=1.0, resid=None):
    """+bias -> ReLU -> gate (gate > 0 ? x * gate_scale : 0) -> dropout (mask ? x * drop_scale : 0) -> +resid, in prod's dtype."""
    x = prod
    if bias is not None:
        x = x + bias.to(x.dtype)
    if relu:
        x = torch.relu(x)
    if gate is not None:
        x = torch.where(gate > 0, x * gate_scale, torch.zeros_like(x))
    if mask is not None:
        x = torch.where(mask > 0, x * drop_scale, torch.zeros_like(x))
    if resid is not None:
        x = x + resid.to(x.dtype)
    return x


# ------------------------------------------------------------------------------------------------ errors and yardsticks
def magnitude(A, B, bias=None, resid=None):
    """(|A| |B|^T + |bias| + |resid|) in float64: the denominator of the componentwise error."""
    d = A.double().abs() @ B.double().abs().T
    if bias is not None:
        d = d + bias.double().abs()
    if resid is not None:
        d = d + resid.double().abs()
    return d


def comp_err(got, ref, mag):
    """max |got - ref| / mag.  A NaN, or anything but zero where the magnitude is zero, is an infinite error."""
    got, ref, mag = [torch.as_tensor(t).detach().double().cpu() for t in (got, ref, mag)]
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    d = (got - ref).abs()
    e = torch.where(mag > 0, d / mag.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    return float(e.max()) if e.numel() else 0.0


def bound(e_fmt, e_fp32):
    return max(CHAIN_FACTOR * (e_fmt + e_fp32), TOL_FP32)


def yardsticks(A, B, precision, family="planes", **epi):
    """One float product with its epilogue: dict(ref, mag, e_fmt, e_fp32, bound), and the same for rowsum_a under "rs_"."""
    split = split_of(family, precision)
    Ad, Bd = A.double(), B.double()
    mag = magnitude(A, B, epi.get("bias"), epi.get("resid"))
    ref = epilogue(Ad @ Bd.T, **epi)
    e_fmt = comp_err(epilogue(fmt_matmul(Ad, Bd.T, precision, split), **epi), ref, mag)
    e_fp32 = comp_err(epilogue(fp32_tiled(A, B), **epi), ref, mag)
    rs_ref, rs_mag = Ad.sum(1), Ad.abs().sum(1)
    rs_fmt = comp_err(expected_rowsum(A, precision, split), rs_ref, rs_mag)
    rs_fp32 = comp_err(A.float().sum(1), rs_ref, rs_mag)
    return dict(ref=ref, mag=mag, e_fmt=e_fmt, e_fp32=e_fp32, bound=bound(e_fmt, e_fp32),
                rs_ref=rs_ref, rs_mag=rs_mag, rs_e_fmt=rs_fmt, rs_e_fp32=rs_fp32, rs_bound=bound(rs_fmt, rs_fp32))


# ------------------------------------------------------------------------------------------------ mutants
def mutants(A, B, precision, split=kr.bf16_split, nks=2):
    """{name: float64 product of a subtly wrong kernel}, built from the reference's own passes; only the ones that apply to this
    precision and K.  tests/test_gemm_ref_cpu.py holds the integer equality and the float bound against each."""
    M, K = A.shape
    exp = expected(A, B, precision, split)
    last = slice((ktiles(K) - 1) * KT, K)                    # the last 64-k tile
    octet = slice(max(K - 8, 0), K)                          # the last k-octet
    out = {}
    if precision >= 2:
        _, hl, lh, _ = passes(A[:, last], B[:, last], split)
        out["the A_hi B_lo pass lost on the last 64-k tile"] = exp - hl
        if precision == 3:
            out["the A_lo B_hi pass lost on the last 64-k tile"] = exp - lh
        _, hl, lh, _ = passes(A[:, octet], B[:, octet], split)
        out["both tails of the last k-octet lost"] = exp - hl - (lh if precision == 3 else 0)
        row = exp.clone()
        row[M - 1] = expected(A[M - 1:], B, 1, split)[0]
        out["the last row run with one pass"] = row
    if precision == 1:
        out["the last k element dropped"] = expected(A[:, :K - 1], B[:, :K - 1], 1, split) if K > 1 else torch.zeros_like(exp)
        out["one extra pass"] = exp + passes(A, B, split)[2]
    if ktiles(K) >= 2:
        nks = min(nks, ktiles(K))
        t = ktiles(K) // nks - 1                             # the last tile of the first slice
        out["K short by one tile in one split-K slice"] = exp - expected(A[:, t * KT:(t + 1) * KT], B[:, t * KT:(t + 1) * KT], precision, split)
    return out
