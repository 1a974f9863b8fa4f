"""The plane GEMM's epilogue (csrc/gemm_planes.hip, plane_tile) on the tiles whose K loop runs in two parts with epilogue work
between them: the 96 x 64 tile makes its dropout decisions between the ring's prologue and the loop and takes phase 1b through
its accumulators in registers, one step of the chain at a time.  Every case runs with the tile forced to 96 x 64, 64 x 64 and
128 x 128 and must give the same bits at all three; cases a, b, c and e are also recomputed from the raw product of the same job
(no epilogue) with the same fp32 operations in the same order in torch, and must be EQUAL: the epilogue is element-wise, every
operation is rounded on its own, and an LDS round trip keeps the compiler from contracting across it.  K = 64, 128, 512: a K
loop shorter than, as long as and longer than the ring's prefetch distance -- whatever is requested between the ring's stages
shares the DMA's counted waits, and a wait that is too short shows up as wrong bits."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

M = 208                                     # two whole 96-row tiles and a partial one
TILES = (96, 64, 128)
GEO = {96: 4, 64: 0, 128: 1}
P_DROP, SITE = 0.25, 3


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    return o


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


@contextlib.contextmanager
def tile(knob):
    from slnlp._lib import load, check
    try:
        check(load().slnlp_set_plane_tile(knob), "set_plane_tile")
        yield
    finally:
        load().slnlp_set_plane_tile(0)


def at_every_tile(ops, run, what, solo=True):
    """run() -> (job, [outputs]) launched at each forced tile: the outputs of the first, after holding the others to its bits."""
    first = None
    for knob in TILES:
        with tile(knob):
            j, outs, launch = run()
            if solo:
                assert ops.plane_geo([j]) == GEO[knob], (what, "forced tile not taken", knob)
            launch()
            torch.cuda.synchronize()
        if first is None:
            first = outs
        else:
            assert len(outs) == len(first)
            for i, (a, b) in enumerate(zip(outs, first)):
                assert torch.equal(a, b), f"{what}: output {i} at tile {knob} differs from tile {TILES[0]}"
    return first


@pytest.fixture(scope="module")
def operands():
    """A [208, 512], B [192, 512], bias, residual, gate once: every case takes its corner."""
    return dict(A=rnd(M, 512, seed=1), B=rnd(192, 512, seed=2), bias=rnd(192, seed=3), R=rnd(M, 192, seed=4), G=rnd(M, 192, seed=5))


def planes_of(v):
    """(hi, lo) of an fp32 tensor as the library splits it: hi = bf16(v), lo = bf16(v - hi), both round-to-nearest-even."""
    hi = v.bfloat16()
    lo = (v - hi.float()).bfloat16()
    return hi.view(torch.int16), lo.view(torch.int16)


@pytest.mark.parametrize("layout,precision", [("forward", 3), ("dgrad", 2)])
@pytest.mark.parametrize("K", [64, 128, 512])
@pytest.mark.parametrize("N", [192, 72])
def test_epilogues_same_bits_at_every_tile_and_as_recomputed(ops, operands, N, K, layout, precision):
    A, B = operands["A"][:, :K].contiguous().cuda(), operands["B"][:N, :K].contiguous().cuda()
    bias, R, G = operands["bias"][:N].cuda(), operands["R"][:, :N].contiguous().cuda(), operands["G"][:, :N].contiguous().cuda()
    Ap = ops.split_planes(A)
    Bp = ops.split_planes(B) if layout == "forward" else ops.split_planes(B.T.contiguous())
    rng = ops.make_rng(seed=7, step=5)
    gscale = 1.0 / (1.0 - P_DROP)
    what = (layout, precision, N, K)

    def job(*, bias_=None, relu=False, resid=None, in_place=False, gate=False, drop=False, planes=None, no_c=False):
        def run():
            out = R.clone() if in_place else torch.full((M, N), float("nan"), device="cuda")
            j, _ = ops.plane_job(Ap, Bp, M=M, N=N, K=K, b_kmajor=layout == "forward", precision=precision, out=out, bias=bias_,
                                 relu=relu, resid=out if in_place else resid)
            outs = [] if no_c else [out]
            if no_c:
                j.C = None
            if gate:
                j.gate, j.ldg, j.gate_scale, j.gate_mode = G.data_ptr(), G.stride(0), gscale, 0
            if drop:
                j.drop_p, j.drop_site, j.rng = P_DROP, SITE, rng.data_ptr()
            if planes:
                cp = ops.split_planes(torch.zeros(M, N).cuda())
                j.C_hi, j.ldc_p = cp[0].data_ptr(), cp[0].stride(0)
                outs.append(cp[0][:M, :N])
                if planes == "hi+lo":
                    j.C_lo = cp[1].data_ptr()
                    outs.append(cp[1][:M, :N])
                keep.append(cp)
            return j, outs, lambda: ops.gemm_group([j], [1])
        keep = []
        return at_every_tile(ops, run, what)

    raw, = job()
    # (a) bias + residual in place
    out, = job(bias_=bias, in_place=True)
    assert torch.equal(out, (raw + bias) + R), (what, "a")
    # (b) residual whose row stride is not C's
    wide = torch.zeros(M, N + 8, device="cuda")
    wide[:, :N] = R
    out, = job(resid=wide[:, :N])
    assert torch.equal(out, raw + R), (what, "b")
    # (c) late route: ReLU gate with scale, then the residual; no dropout
    out, = job(gate=True, resid=R)
    scaled = raw * torch.tensor(gscale, dtype=torch.float32, device="cuda")
    assert torch.equal(out, torch.where(G > 0, scaled, torch.zeros_like(raw)) + R), (what, "c")
    # (d) early route: ReLU + dropout + gate + `also` planes -- the mask is the library's own: held across the tiles only
    out, hi, lo = job(bias_=bias, relu=True, gate=True, drop=True, planes="hi+lo")
    whi, wlo = planes_of(out)
    assert torch.equal(hi, whi) and torch.equal(lo, wlo), (what, "d: the planes are the split of the fp32 result")
    # (ReLU and the gate each pass about half -- the bias is small beside a product of K terms -- and dropout keeps 3 / 4: 0.19)
    assert 0.12 < float((out != 0).float().mean()) < 0.25, (what, "d: share of live elements")
    # (e) planes only, hi and lo, and hi alone
    whi, wlo = planes_of(raw)
    hi, lo = job(planes="hi+lo", no_c=True)
    assert torch.equal(hi, whi) and torch.equal(lo, wlo), (what, "e")
    hi, = job(planes="hi", no_c=True)
    assert torch.equal(hi, whi), (what, "e, hi alone")


def grad_jobs(ops, T, No, Ki, with_resid):
    dY, X, W, R = rnd(T, No, seed=11).cuda(), rnd(T, Ki, seed=12).cuda(), rnd(No, Ki, seed=13).cuda(), rnd(T, Ki, seed=14).cuda()
    dYp, Xp, Wp = ops.split_planes(dY), ops.split_planes(X), ops.split_planes(W)
    def make():
        rs = torch.full((No,), float("nan"), device="cuda")
        dW, dX = torch.full((No, Ki), float("nan"), device="cuda"), torch.full((T, Ki), float("nan"), device="cuda")
        jw, _ = ops.plane_job(dYp, Xp, M=No, N=Ki, K=T, a_kmajor=False, b_kmajor=False, precision=2, rowsum_a=rs, out=dW)
        jd, _ = ops.plane_job(dYp, Wp, M=T, N=Ki, K=No, b_kmajor=False, precision=2, out=dX, resid=R if with_resid else None)
        return jw, jd, [dW, rs, dX]
    return make, (dY, X, W, R)


def test_split_k_early_return_same_bits_at_64_and_128(ops):
    """A weight gradient in three K-slices with the bias gradient's row sums: the workgroups that are not the last to arrive leave
    before the epilogue, and the last one adds the residual in place (accumulation into dW)."""
    T, No, Ki = 320, 192, 72
    dY, X, acc0 = rnd(T, No, seed=21).cuda(), rnd(T, Ki, seed=22).cuda(), rnd(No, Ki, seed=23).cuda()
    dYp, Xp = ops.split_planes(dY), ops.split_planes(X)
    res = {}
    for knob in (64, 128):
        with tile(knob):
            rs, dW = torch.full((No,), float("nan"), device="cuda"), acc0.clone()
            j, _ = ops.plane_job(dYp, Xp, M=No, N=Ki, K=T, a_kmajor=False, b_kmajor=False, rowsum_a=rs, out=dW, resid=dW)
            assert ops.plane_geo([j], [3]) == GEO[knob]
            ops.gemm_group([j], [3])
            torch.cuda.synchronize()
            res[knob] = (dW, rs)
    assert torch.equal(res[64][0], res[128][0]) and torch.equal(res[64][1], res[128][1])
    want = dY.double().T @ X.double() + acc0.double()
    assert float((res[64][0].double() - want).abs().max() / want.abs().max()) < 1e-4     # three-pass split-bf16 (test_kernels_gpu.py)
    assert float((res[64][1].double() - dY.double().sum(0)).abs().max() / dY.double().sum(0).abs().max()) < 1e-4


def test_grouped_pair_only_the_data_gradient_has_a_residual(ops):
    """ops.gemm_wd as the training plans launch a gradient pair, against the two jobs launched apart with the split it chose."""
    make, keep = grad_jobs(ops, 208, 192, 72, with_resid=True)
    jw, jd, together = make()
    split = ops.gemm_wd_plan(jw, jd)[0]
    ops.gemm_wd(jw, jd)
    jw, jd, apart = make()
    ops.gemm_group([jw], [split])
    ops.gemm_group([jd], [1])
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(together, apart)):
        assert not torch.isnan(a).any()
        assert torch.equal(a, b), f"output {i} of the grouped pair differs from the jobs launched apart"
