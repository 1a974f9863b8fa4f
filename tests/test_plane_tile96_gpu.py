"""The plane GEMM's 96 x 64 tile (geometry 4, csrc/gemm_planes.hip): a 2 (M) x 4 (N) wave grid over an A panel of one and a
half plane images, chosen for solo launches that are more than one workgroup per CU at 64 x 64 and at most one at 96 x 64.
include/slnlp.h promises that results do not depend on the tile: every case here runs with the tile forced to 96 x 64 and again
forced to 64 x 64 and holds the two bit for bit, and to an fp64 torch product within the tolerance test_kernels_gpu.py uses for
that precision (1e-4 of the largest element: three-pass split-bf16, and two-pass against the product of bf16(dY))."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MS, NS, KS = (50, 96, 112, 208), (64, 80, 192), (64, 128, 512, 1536)   # < one tile, exact, ragged by one MFMA block, two tiles + ragged
TOL = 1e-4


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    return o


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


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


def at_both_tiles(run):
    """run() at the 96 x 64 tile, then at 64 x 64: ([outputs], [outputs])."""
    with tile(96):
        got = run()
        torch.cuda.synchronize()
    with tile(64):
        ref = run()
        torch.cuda.synchronize()
    return got, ref


def same_bits(got, ref, what):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), f"{what}: output {i} differs between the 96 x 64 and the 64 x 64 tile"


@pytest.fixture(scope="module")
def operands(ops):
    """(A [208, 1536], B [192, 1536]) once: every case takes its M x K / N x K corner."""
    return rnd(max(MS), max(KS), seed=1), rnd(max(NS), max(KS), seed=2)


@pytest.mark.parametrize("layout,precision", [("forward", 3), ("dgrad", 3), ("dgrad", 2)])
def test_every_shape_keeps_the_bits_of_the_64_tile(ops, operands, layout, precision):
    """Forward layout (both operands k-major), data-gradient layout (B m-major) at three passes, and the two-pass backward
    setting (precision 2: A enters with its bf16 head)."""
    A_all, B_all = operands
    for M, N, K in itertools.product(MS, NS, KS):
        A, B = A_all[:M, :K].contiguous().cuda(), B_all[:N, :K].contiguous().cuda()
        Ap = ops.split_planes(A)
        Bp = ops.split_planes(B) if layout == "forward" else ops.split_planes(B.T.contiguous())
        def run():
            j, out = ops.plane_job(Ap, Bp, M=M, N=N, K=K, b_kmajor=layout == "forward", precision=precision)
            out.fill_(float("nan"))
            if ops.plane_geo([j]) == 4:
                geos.append(4)
            ops.gemm_group([j], [1])
            return [out]
        geos = []
        got, ref = at_both_tiles(run)
        assert geos == [4], "the forced 96 x 64 tile was not taken"
        same_bits(got, ref, (layout, precision, M, N, K))
        want = (A.bfloat16().double() if precision == 2 else A.double()) @ B.double().T
        assert rel(got[0], want) < TOL, (layout, precision, M, N, K)


@pytest.mark.parametrize("M,N,K", [(208, 192, 512), (112, 80, 128), (50, 64, 64), (130, 70, 100)])
def test_epilogues_one_at_a_time_and_together(ops, M, N, K):
    """bias; ReLU + dropout + `also` planes; residual `plus`; rowsum_a -- each alone, then all on one job.  The dropout mask is a
    function of the element's global (row, column): the 2 x 4 wave grid splits a Philox call's column pair over two waves."""
    A, B, bias, R = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3).cuda(), rnd(M, N, seed=4).cuda()
    pad = lambda x: torch.nn.functional.pad(x, (0, (-x.shape[1]) % 4))
    Ap, Bp = ops.split_planes(pad(A).cuda()), ops.split_planes(pad(B).cuda())
    rng, p, site = ops.make_rng(seed=7, step=5), 0.25, 3
    prod = A.double().cuda() @ B.double().cuda().T
    mask = ops.dropout_mask(M, N, p, site, rng) > 0
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))

    def job(bias_=None, relu=False, drop=False, planes=False, resid=None, rowsum=False):
        def run():
            rs = torch.full((M,), float("nan"), device="cuda") if rowsum else None
            j, out = ops.plane_job(Ap, Bp, M=M, N=N, K=K, bias=bias_, relu=relu, resid=resid, rowsum_a=rs)
            out.fill_(float("nan"))
            outs = [out]
            if drop:
                j.drop_p, j.drop_site, j.rng = p, site, rng.data_ptr()
            if planes:
                cp = ops.split_planes(torch.zeros(M, (N + 3) // 4 * 4).cuda())
                j.C_hi, j.C_lo, j.ldc_p = cp[0].data_ptr(), cp[1].data_ptr(), cp[0].stride(0)
                outs += [cp[0], cp[1]]
            if rowsum:
                outs.append(rs)
            assert ops.plane_geo([j]) in (0, 4)
            ops.gemm_group([j], [1])
            return outs
        got, ref = at_both_tiles(run)
        same_bits(got, ref, (M, N, K, bias_ is not None, relu, drop, planes, resid is not None, rowsum))
        return got

    zero = torch.zeros((), dtype=torch.float64, device="cuda")
    out, = job(bias_=bias)
    assert rel(out, prod + bias.double()) < TOL
    out, hi, lo = job(relu=True, drop=True, planes=True)
    want = torch.where(mask, torch.relu(prod) * scale, zero)
    assert rel(out, want) < TOL
    whi, wlo = ops.split_planes(pad(out))
    assert torch.equal(hi[:M, :N], whi[:M, :N]) and torch.equal(lo[:M, :N], wlo[:M, :N])      # the planes are the split of the fp32 result
    out, = job(resid=R)
    assert rel(out, prod + R.double()) < TOL
    out, rs = job(rowsum=True)
    assert rel(out, prod) < TOL and rel(rs, A.double().sum(1)) < TOL
    out, hi, lo, rs = job(bias_=bias, relu=True, drop=True, planes=True, resid=R, rowsum=True)
    want = torch.where(mask, torch.relu(prod + bias.double()) * scale, zero) + R.double()
    assert rel(out, want) < TOL and rel(rs, A.double().sum(1)) < TOL
    whi, wlo = ops.split_planes(pad(out))
    assert torch.equal(hi[:M, :N], whi[:M, :N]) and torch.equal(lo[:M, :N], wlo[:M, :N])


def train_step_state(c, knob, dropout=0.1):
    """One train step of a fresh TransformerEngine under tile knob `knob` (0: the library's own rule): (loss, grad norm, params, log-probs)."""
    from slnlp import synth, tf_engine as te
    from oracle import transformer_ref as tr
    shapes = tr.param_shapes(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"])
    sd = {k: torch.from_numpy(v) for k, v in synth.make_weights(shapes, seed=1).items()}
    X, _, y = [torch.from_numpy(a) for a in synth.make_batch(c["B"], c["S"], c["Vs"], c["Vt"], seed=1, min_len=3)]
    with tile(knob):
        eng = te.TransformerEngine(te.make_config(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"], c["B"], c["S"], dropout=dropout), device="cuda:0", seed=3)
        eng.load_state(sd)
        eng.set_lr(0.01)
        logp = eng.train_step(X.cuda(), y.cuda()).clone()
        torch.cuda.synchronize()
        return eng.loss, eng.grad_norm, eng.params.clone(), logp


def same_step(a, b):
    assert a[0] == b[0] and a[1] == b[1], ("loss / grad norm", a[:2], b[:2])
    assert torch.equal(a[2], b[2]), "parameters differ after one train step"
    assert torch.equal(a[3], b[3]), "log-probs differ"


def test_plan_below_the_rule_forced_tile(ops):
    """A Transformer plan of 288 rows: the rule does not fire, the forced knob puts every solo k-major launch on the 96 x 64 tile."""
    c = dict(Vs=64, Vt=16, E=64, H=2, N=1, F=64, B=6, S=48)
    j, _ = ops.plane_job((torch.zeros(1), torch.zeros(1)), (torch.zeros(1), torch.zeros(1)), M=288, N=64, K=64, out=torch.zeros(1))
    assert ops.plane_geo([j]) == 0
    same_step(train_step_state(c, 96), train_step_state(c, 64))


def test_plan_inside_the_rule_window(ops):
    """2400 rows x F = 512: linear1's forward product and linear2's data gradient are 304 workgroups at 64 x 64 and 200 at 96 x 64 --
    the rule fires by itself.  One train step with the rule on and one with the 64 x 64 tile forced: the same step."""
    c = dict(Vs=64, Vt=16, E=128, H=2, N=1, F=512, B=50, S=48)
    j, _ = ops.plane_job((torch.zeros(1), torch.zeros(1)), (torch.zeros(1), torch.zeros(1)), M=2400, N=512, K=128, out=torch.zeros(1))
    assert ops.plane_geo([j]) == 4
    same_step(train_step_state(c, 0), train_step_state(c, 64))
