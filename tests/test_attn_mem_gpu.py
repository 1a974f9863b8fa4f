"""GPU parity of the decoder's cross-attention over the unprojected memory (csrc/attention_mem.hip), stage by stage against
kernel_refs.xmem_ref in float64: the forward and backward kernels at 1 / 2 / 4 heads per workgroup (same bits), the per-row d
memory kernel and its all-layers form, and the batched per-head GEMM jobs around them (csrc/linear_jobs.hpp), alone and as the
plan chains them.  Bounds are the project's for fp32 attention kernels (test_kernels_gpu.py::test_attn_cross): 2e-5 of the tensor
maximum for forward outputs, 5e-5 for backward outputs; precision-3 products TOL[3] * max(1, sqrt(K / 64)); the composed block 1e-4.

Every kernel output lives inside one larger buffer filled with a sentinel, 64 floats of guard on either side, its interior
pre-filled with NaN: a store outside an output or an element left unwritten shows.

SLNLP_ATTN_MEM_PROFILE=<path>: also write the per-output maxima of the measured errors there (profiles/attn_mem_parity.json)."""
import functools
import json
import math
import os

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_BWD, TOL_BLOCK, TOL3 = 2e-5, 5e-5, 1e-4, 5e-5
GUARD, SENTINEL = 64, -1.2345678e30
SEED, STEP, SITE = 8, 1, 9

# (B, S, H, dh): each the smallest shape that reaches a distinct branch
SHAPES = [(50, 48, 8, 64),      # the benchmark's; E = 512: two row sets in the d-memory kernel; grid % 8 == 0: xcd_local permutes
          (3, 13, 3, 8),        # odd H: the 1-head kernels, the repeated last head; E = 24: 10 row sets, 16 idle threads; S % 4, % 8 != 0
          (5, 70, 4, 16),       # S > 64: the softmax lane loops; more than one row_dots_multi trip of 24 rows
          (2, 1, 2, 4),         # S = 1, dh = 4, E = 8: two active lanes
          (4, 27, 1, 64),       # H = 1
          (2, 9, 8, 128),       # E = 1024: sets == 1, every thread owns a column chunk
          (3, 25, 5, 32),       # E = 160: 6 row sets do not divide 8 rows
          (2, 11, 64, 4),       # H = XMEM_MAX_HEADS
          (8, 24, 2, 32),       # grid % 8 == 0 at one and at two heads per workgroup; S = 24: exactly one trip
          (4, 200, 4, 256)]     # E = 1024 with S > 3 * 64
assert SHAPES[1:5] == kr.XMEM_SHAPES

MEASURED = {}


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    yield o
    path = os.environ.get("SLNLP_ATTN_MEM_PROFILE")
    if path and MEASURED:
        doc = {"what": "tests/test_attn_mem_gpu.py on an MI355X: max |kernel - fp64 reference| / max |reference| per output, the maximum over all cases",
               "bounds": {"forward": TOL_FWD, "backward": TOL_BWD, "dmem_all": "5e-5 * sqrt(N)", "head_jobs": "5e-5 * max(1, sqrt(K / 64))",
                          "block": TOL_BLOCK},
               "max_error_over_all_cases": {k: {n: float(f"{v:.3e}") for n, v in sorted(d.items())} for k, d in sorted(MEASURED.items())}}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def err(got, ref):
    """max |got - ref| / max |ref| in float64; a reference that is exactly zero admits exactly zero only."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else math.inf
    return float((got - ref).abs().max()) / top


def note(group, case, name, e, bound):
    print(f"{group} {case} {name}: {e:.2e} (bound {bound:.1e})")
    d = MEASURED.setdefault(group, {})
    if math.isfinite(e):
        d[name] = max(d.get(name, 0.0), e)
    return e


class Guarded:
    """Named float32 outputs inside ONE sentinel-filled device buffer: GUARD floats on either side of each (interiors rounded up
    to 4 floats, the tail counted as guard), interiors NaN."""

    def __init__(self, **shapes):
        off, self.spans = GUARD, {}
        for name, shape in shapes.items():
            n = math.prod(shape)
            self.spans[name] = (off, n, shape)
            off += (n + 3) // 4 * 4 + GUARD
        self.buf = torch.full((off,), SENTINEL, dtype=torch.float32, device="cuda")
        inside = torch.zeros(off, dtype=torch.bool)
        for o, n, _ in self.spans.values():
            inside[o:o + n] = True
        self.outside = (~inside).cuda()
        self.buf[~self.outside] = float("nan")

    def __getitem__(self, name):
        o, n, shape = self.spans[name]
        return self.buf[o:o + n].view(shape)

    def fill(self, name, values):
        self[name].copy_(values)

    def check(self, nan_free=True):
        """every guard float untouched; no NaN left in any output"""
        torch.cuda.synchronize()
        assert bool((self.buf[self.outside] == SENTINEL).all()), "a guard float was overwritten"
        for name in self.spans if nan_free else ():
            assert not bool(torch.isnan(self[name]).any()), f"{name}: NaN left (an element was not written, or a NaN was computed)"


def fwd_outputs(B, S, H, dh):
    E = H * dh
    return Guarded(mbar=(B * H, E), psum=(B * H,), probs=(B * H, S), ctx0=(B, E))


def bwd_outputs(B, S, H, dh):
    E = H * dh
    return Guarded(dsc=(B * H, S), dqk=(B * H, E), dcp=(B, E), dbv=(E,), dmem=(S * B, E))


def run_fwd(ops, dev, shape, p, rng, site=SITE):
    B, S, H, dh = shape
    g = fwd_outputs(*shape)
    ops.attn_mem_fwd(dev["qk"], dev["mem"], dev["bv"], B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=site, rng=rng,
                     out=(g["mbar"], g["psum"], g["probs"], g["ctx0"]))
    return g


def run_bwd(ops, dev, probs, psum, shape, p, rng, site=SITE, start=None):
    """start None: d memory written (accumulate = 0) over its NaN prefill; else added (accumulate = 1) onto `start`"""
    B, S, H, dh = shape
    g = bwd_outputs(*shape)
    if start is not None:
        g.fill("dmem", start)
    ops.attn_mem_bwd(dev["mem"], dev["bv"], probs, psum, dev["qk"], dev["dmbar"], dev["dctx"], B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=site,
                     rng=rng, dmem=g["dmem"], accumulate=start is not None, out=(g["dsc"], g["dqk"], g["dcp"], g["dbv"]))
    return g


def keep_mask(ops, B, S, H, p, site, rng):
    return ops.dropout_mask(B * H, S, p, site, rng).cpu().double() if p > 0 else None


@functools.lru_cache(maxsize=None)
def case(shape, p):
    """(float32 inputs, dropout keep-mask as the library reports it, float64 reference), computed once per (shape, p)"""
    from slnlp import ops
    B, S, H, dh = shape
    inp = kr.xmem_inputs(*shape)
    mask = keep_mask(ops, B, S, H, p, SITE, ops.make_rng(seed=SEED, step=STEP))
    ref = kr.xmem_ref(B=B, S=S, H=H, dh=dh, mask=mask, p=p, **{k: v.double() for k, v in inp.items()})
    return inp, mask, ref


# ------------------------------------------------------------------------------------------------- (a) parity per stage
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_each_stage_against_fp64(ops, shape, p):
    """forward: probs, psum, mbar, ctx0; backward, fed the REFERENCE's probs and psum (a forward error can neither mask nor cause
    a backward one): dsc, dqk, dcp, dbv and d memory, written over NaN and added onto a random start."""
    B, S, H, dh = shape
    inp, mask, ref = case(shape, p)
    dev = {k: v.cuda() for k, v in inp.items()}
    rng = ops.make_rng(seed=SEED, step=STEP)
    f = run_fwd(ops, dev, shape, p, rng)
    f.check()
    errs = {n: note("forward", (shape, p), n, err(f[n], ref[n]), TOL_FWD) for n in ("probs", "psum", "mbar", "ctx0")}
    probs, psum = ref["probs"].float().cuda(), ref["psum"].float().cuda()
    b = run_bwd(ops, dev, probs, psum, shape, p, rng)
    b.check()
    berrs = {n: note("backward", (shape, p), n, err(b[n], ref[n]), TOL_BWD) for n in ("dsc", "dqk", "dcp", "dbv", "dmem")}
    start = torch.randn(S * B, H * dh, generator=torch.Generator().manual_seed(4))
    b2 = run_bwd(ops, dev, probs, psum, shape, p, rng, start=start.cuda())
    b2.check()
    berrs["dmem_accumulated"] = note("backward", (shape, p), "dmem_accumulated", err(b2["dmem"], start.double() + ref["dmem"]), TOL_BWD)
    for n in ("dsc", "dqk", "dcp", "dbv"):
        assert torch.equal(b2[n], b[n]), n
    if S == 1:
        assert torch.equal(f["probs"], torch.ones_like(f["probs"])) and torch.equal(b["dsc"], torch.zeros_like(b["dsc"]))
    if p > 0:
        assert float((ref["psum"] - 1).abs().max()) > 0.05              # the mask is live
    for n, e in errs.items():
        assert e < TOL_FWD, (n, e)
    for n, e in berrs.items():
        assert e < TOL_BWD, (n, e)


# ------------------------------------------------------------------------------- (b) heads per workgroup: the same bits
def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", [SHAPES[i] for i in (0, 2, 5, 7, 8, 1)], ids=lambda s: "x".join(map(str, s)))
def test_heads_per_workgroup_return_the_same_bits(ops, shape):
    """slnlp_set_xmem_heads(1 / 2 / 4): every output of forward and backward bit for bit; a forced value that does not divide H
    (H = 3) or exceeds it (H = 2 at 4) falls back and still succeeds."""
    B, S, H, dh = shape
    p = 0.25
    inp, _, ref = case(shape, p)
    dev = {k: v.cuda() for k, v in inp.items()}
    rng = ops.make_rng(seed=SEED, step=STEP)
    got = {}
    try:
        for hp in (1, 2, 4):
            ops.set_xmem_heads(hp)
            f = run_fwd(ops, dev, shape, p, rng)
            b = run_bwd(ops, dev, f["probs"], f["psum"], shape, p, rng)
            f.check()
            b.check()
            got[hp] = {**{n: f[n].clone() for n in f.spans}, **{n: b[n].clone() for n in b.spans}}
    finally:
        ops.set_xmem_heads(0)
    for n, t in got[1].items():
        bound = TOL_FWD if n in ("mbar", "psum", "probs", "ctx0") else TOL_BWD
        if n in ref and n not in ("dsc", "dqk", "dmem"):            # (those three follow the kernel's own fp32 probs here)
            assert err(t, ref[n]) < bound, n
        for hp in (2, 4):
            assert torch.equal(bits(got[hp][n]), bits(t)), f"{n}: {hp} heads per workgroup differ from 1"


# ------------------------------------------------------------------------------------- (c) one launch for all layers
def layer_masks(ops, B, S, H, p, sites, rng):
    return [keep_mask(ops, B, S, H, p, s, rng) for s in sites]


def dmem_ref(layers, masks, B, S, H, dh, p):
    E = H * dh
    tot = torch.zeros(S, B, E, dtype=torch.float64)
    for L, m in zip(layers, masks):
        pd = (L["probs"].double().cpu() * m / (1 - p)).view(B, H, S)
        tot += torch.einsum("bhs,bhe->sbe", pd, L["dmbar"].double().cpu().view(B, H, E))
        tot += torch.einsum("bhs,bhe->sbe", L["dsc"].double().cpu().view(B, H, S), L["qk"].double().cpu().view(B, H, E))
    return tot.reshape(S * B, E)


@pytest.mark.parametrize("N", [1, 3, 9])
@pytest.mark.parametrize("shape", [(3, 13, 3, 8), (3, 25, 5, 32), (2, 9, 8, 128)], ids=lambda s: "x".join(map(str, s)))
def test_dmem_of_all_layers_in_one_launch(ops, shape, N):
    """slnlp_attn_mem_dmem_all (N = 9: two staging trips of DMEM_STAGE_LAYERS = 8) over a NaN-prefilled d memory: the fp64 sum
    over layers and heads on tables of random per-layer tensors, every layer's dbv = the column sums of its dcp, and the bits of
    N accumulating slnlp_attn_mem_bwd calls, layers N-1 ... 0."""
    B, S, H, dh = shape
    E, p = H * dh, 0.25
    g = torch.Generator().manual_seed(100 * N + S)
    rnd = lambda *s: torch.randn(*s, generator=g)
    rng = ops.make_rng(seed=SEED, step=STEP)
    sites = [20 + 3 * l for l in range(N)]
    masks = layer_masks(ops, B, S, H, p, sites, rng)
    bound = TOL_BWD * math.sqrt(N)

    # (1) every table entry random: probs a softmax, the rest unit scale
    outs = Guarded(dmem=(S * B, E), **{f"dbv{l}": (E,) for l in range(N)})
    layers = [dict(probs=torch.softmax(rnd(B * H, S), -1).cuda(), dsc=rnd(B * H, S).cuda(), dmbar=rnd(B * H, E).cuda(), qk=rnd(B * H, E).cuda(),
                   dcp=rnd(B, E).cuda(), dbv=outs[f"dbv{l}"], drop_site=sites[l]) for l in range(N)]
    _, table = ops.attn_mem_dmem_all(layers, B=B, S=S, H=H, dh=dh, drop_p=p, rng=rng, dmem=outs["dmem"])
    outs.check()
    e = err(outs["dmem"], dmem_ref(layers, masks, B, S, H, dh, p))
    note("dmem_all", (shape, N), "dmem_over_sqrt_N", e / math.sqrt(N), TOL_BWD)
    assert e < bound
    for l, L in enumerate(layers):
        e = note("dmem_all", (shape, N), "dbv", err(L["dbv"], L["dcp"].double().cpu().sum(0)), TOL_BWD)
        assert e < TOL_BWD, l

    # (2) the tables that N backward calls leave: the chained launches and the one launch agree bit for bit
    mem = rnd(S * B, E).cuda()
    chain = Guarded(dmem=(S * B, E))
    per_layer, tab = [None] * N, [None] * N
    for l in range(N - 1, -1, -1):
        dev = dict(mem=mem, bv=rnd(E).cuda(), qk=(rnd(B * H, E) * math.sqrt(dh / E)).cuda(), dmbar=rnd(B * H, E).cuda(), dctx=rnd(B, E).cuda())
        probs = torch.softmax(rnd(B * H, S), -1)
        psum = (probs.double() * masks[l] / (1 - p)).sum(-1).float()
        b = Guarded(dsc=(B * H, S), dqk=(B * H, E), dcp=(B, E), dbv=(E,), dbv_all=(E,))
        ops.attn_mem_bwd(dev["mem"], dev["bv"], probs.cuda(), psum.cuda(), dev["qk"], dev["dmbar"], dev["dctx"], B=B, S=S, H=H, dh=dh, drop_p=p,
                         drop_site=sites[l], rng=rng, dmem=chain["dmem"], accumulate=l != N - 1, out=(b["dsc"], b["dqk"], b["dcp"], b["dbv"]))
        per_layer[l] = b
        tab[l] = dict(probs=probs.cuda(), dsc=b["dsc"], dmbar=dev["dmbar"], qk=dev["qk"], dcp=b["dcp"], dbv=b["dbv_all"], drop_site=sites[l])
    chain.check()
    one = Guarded(dmem=(S * B, E))
    _, table2 = ops.attn_mem_dmem_all(tab, B=B, S=S, H=H, dh=dh, drop_p=p, rng=rng, dmem=one["dmem"])
    one.check()
    assert torch.equal(bits(one["dmem"]), bits(chain["dmem"]))
    e = err(one["dmem"], dmem_ref(tab, masks, B, S, H, dh, p))
    note("dmem_all", (shape, N), "dmem_after_backward_calls_over_sqrt_N", e / math.sqrt(N), TOL_BWD)
    assert e < bound
    for l in range(N):
        per_layer[l].check()
        assert torch.equal(bits(per_layer[l]["dbv_all"]), bits(per_layer[l]["dbv"])), l
        assert err(per_layer[l]["dbv"], per_layer[l]["dcp"].double().cpu().sum(0)) < TOL_BWD, l
    del table, table2


# ------------------------------------------------------------------------- (d) sequences do not leak into each other
@pytest.mark.parametrize("shape", [(8, 24, 2, 32), (3, 13, 3, 8)], ids=lambda s: "x".join(map(str, s)))
def test_a_nan_sequence_stays_in_its_own_outputs(ops, shape):
    """All inputs of sequence b0 NaN: every output element of another sequence keeps its bits (dbv, a sum over b, excepted),
    every output element of b0 is NaN -- a slip in the bh / xcd_local / row-set indexing cannot average out here."""
    B, S, H, dh = shape
    E, p, b0 = H * dh, 0.25, 1
    inp, _, _ = case(shape, p)
    rng = ops.make_rng(seed=SEED, step=STEP)

    def run(dev):
        f = run_fwd(ops, dev, shape, p, rng)
        b = run_bwd(ops, dev, f["probs"], f["psum"], shape, p, rng)
        torch.cuda.synchronize()
        return f, b

    clean = {k: v.cuda() for k, v in inp.items()}
    bad = {k: v.clone() for k, v in inp.items()}
    nan = float("nan")
    bad["qk"].view(B, H, E)[b0] = nan
    bad["dmbar"].view(B, H, E)[b0] = nan
    bad["dctx"][b0] = nan
    bad["mem"].view(S, B, E)[:, b0] = nan
    f0, g0 = run(clean)
    f1, g1 = run({k: v.cuda() for k, v in bad.items()})
    f0.check()
    g0.check()
    f1.check(nan_free=False)
    g1.check(nan_free=False)
    # each output as [B, ...]: index 0 is the sequence
    by_seq = lambda t, name: t.view(S, B, E).transpose(0, 1) if name == "dmem" else t.view(B, -1)
    for g_clean, g_bad in ((f0, f1), (g0, g1)):
        for name in g_clean.spans:
            if name == "dbv":
                continue
            a, b = by_seq(g_clean[name], name), by_seq(g_bad[name], name)
            others = [i for i in range(B) if i != b0]
            assert torch.equal(bits(a[others]), bits(b[others])), f"{name}: another sequence changed"
            assert bool(torch.isnan(b[b0]).all()), f"{name}: sequence {b0} is not all NaN"


# ----------------------------------------------------------------------------- (e) the batched per-head GEMM jobs
def head_expand_job(x, W, out, B, H, dh):
    """csrc/linear_jobs.hpp head_expand: out[B, H, E] = x_h W_h; x [B, E] (columns h*dh..), W [E, E] (rows h*dh..)"""
    from slnlp._lib import GemmArgs, ptr
    E = H * dh
    a = GemmArgs()
    a.A, a.lda, a.a_kmajor = ptr(x), E, 1
    a.B, a.ldb, a.b_kmajor = ptr(W), E, 0
    a.C, a.ldc, a.M, a.N, a.K = ptr(out), H * E, B, E, dh
    a.ldg, a.ldr, a.precision = E, E, 3
    a.batch, a.batch_stride_a, a.batch_stride_b, a.batch_stride_c = H, dh, dh * E, E
    return a


def head_reduce_job(x, W, out, B, H, dh, resid=None):
    """head_reduce: out[B, E] (columns h*dh..) = x_h W_h^T (+ resid, which may be out itself); x [B, H, E]"""
    from slnlp._lib import GemmArgs, ptr
    E = H * dh
    a = GemmArgs()
    a.A, a.lda, a.a_kmajor = ptr(x), H * E, 1
    a.B, a.ldb, a.b_kmajor = ptr(W), E, 1
    a.C, a.ldc, a.M, a.N, a.K = ptr(out), E, B, dh, E
    a.resid, a.ldr, a.precision = ptr(resid), E, 3
    a.batch, a.batch_stride_a, a.batch_stride_b, a.batch_stride_c = H, E, dh * E, dh
    return a


def head_wgrad_job(dy, x, dW, B, H, dh):
    """head_wgrad: dW_h[dh, E] = dy_h^T x_h; dy [B, E] (columns h*dh..), x [B, H, E], dW [E, E] (rows h*dh..)"""
    from slnlp._lib import GemmArgs, ptr
    E = H * dh
    a = GemmArgs()
    a.A, a.lda, a.a_kmajor = ptr(dy), E, 0
    a.B, a.ldb, a.b_kmajor = ptr(x), H * E, 0
    a.C, a.ldc, a.M, a.N, a.K = ptr(dW), E, dh, E, B
    a.precision = 3
    a.batch, a.batch_stride_a, a.batch_stride_b, a.batch_stride_c = H, dh, E, dh * E
    return a


def launch(ops, jobs):
    ops.gemm_group(jobs, scratch=torch.zeros(16, dtype=torch.uint8, device="cuda"))     # (fp32-operand jobs use no scratch)


def tol3(K):
    return TOL3 * max(1.0, math.sqrt(K / 64))


@pytest.mark.parametrize("B,H,dh", [(50, 8, 64), (3, 3, 8), (7, 1, 64), (5, 5, 32)])
def test_batched_head_jobs_against_fp64(ops, B, H, dh):
    """head_expand, head_reduce (onto an in-place residual, as the plan adds Wv_h mbar onto ctx0) and the backward's grouped
    launch of three (head_reduce + two head_wgrad): batch = H with the strides of linear_jobs.hpp, fp32 operands, precision 3."""
    E = H * dh
    g = torch.Generator().manual_seed(B + H + dh)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x, W, xh, r, dy = rnd(B, E), rnd(E, E), rnd(B, H, E), rnd(B, E), rnd(B, E)
    xd, Wd, xhd, dyd = x.double(), W.double().view(H, dh, E), xh.double(), dy.double()
    o = Guarded(expand=(B, H, E), reduce=(B, E), dq=(B, E), dWk=(E, E), dWv=(E, E))
    o.fill("reduce", r.cuda())
    xc, Wc, xhc, dyc = x.cuda(), W.cuda(), xh.cuda(), dy.cuda()
    launch(ops, [head_expand_job(xc, Wc, o["expand"], B, H, dh)])
    launch(ops, [head_reduce_job(xhc, Wc, o["reduce"], B, H, dh, resid=o["reduce"])])
    launch(ops, [head_reduce_job(xhc, Wc, o["dq"], B, H, dh), head_wgrad_job(xc, xhc, o["dWk"], B, H, dh), head_wgrad_job(dyc, xhc, o["dWv"], B, H, dh)])
    o.check()
    reduce_ref = torch.einsum("bhe,hde->bhd", xhd, Wd).reshape(B, E)
    want = {"expand": (torch.einsum("bhd,hde->bhe", xd.view(B, H, dh), Wd), dh),
            "reduce": (reduce_ref + r.double(), E),
            "dq": (reduce_ref, E),
            "dWk": (torch.einsum("bhd,bhe->hde", xd.view(B, H, dh), xhd).reshape(E, E), B),
            "dWv": (torch.einsum("bhd,bhe->hde", dyd.view(B, H, dh), xhd).reshape(E, E), B)}
    errs = {n: (err(o[n], ref), K) for n, (ref, K) in want.items()}
    for n, (e, K) in errs.items():
        note("head_jobs", (B, H, dh), n + "_over_max_1_sqrt_K_64", e * TOL3 / tol3(K), TOL3)
    for n, (e, K) in errs.items():
        assert e < tol3(K), (n, e, K)


# -------------------------------------------------------------------------- (f) the whole block against the standard form
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("shape", [(50, 48, 8, 64), (3, 13, 3, 8)], ids=lambda s: "x".join(map(str, s)))
def test_block_as_the_plan_chains_it_against_projected_attention(ops, shape, p):
    """expand -> attn_mem_fwd -> reduce onto ctx0; expand -> attn_mem_bwd -> (reduce, wgrad, wgrad), as csrc/tf_plan.hip runs a
    decoder layer's cross-attention, against autograd through kernel_refs.cross_ref on kv = [mem Wk^T + bk | mem Wv^T + bv]."""
    B, S, H, dh = shape
    E = H * dh
    inp = kr.xmem_block_inputs(*shape)
    rng = ops.make_rng(seed=SEED, step=STEP)
    mask = keep_mask(ops, B, S, H, p, SITE, rng)
    std = kr.xmem_block_standard(inp, B, S, H, dh, mask, p)
    d = {k: v.cuda() for k, v in inp.items()}
    o = Guarded(qk=(B * H, E), dmbar=(B * H, E), dq=(B, E), dWk=(E, E), dWv=(E, E))
    launch(ops, [head_expand_job(d["q"], d["Wk"], o["qk"], B, H, dh)])
    f = fwd_outputs(*shape)
    ops.attn_mem_fwd(o["qk"], d["mem"], d["bv"], B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=SITE, rng=rng, out=(f["mbar"], f["psum"], f["probs"], f["ctx0"]))
    launch(ops, [head_reduce_job(f["mbar"], d["Wv"], f["ctx0"], B, H, dh, resid=f["ctx0"])])
    ctx = f["ctx0"]
    launch(ops, [head_expand_job(d["dctx"], d["Wv"], o["dmbar"], B, H, dh)])
    b = bwd_outputs(*shape)
    ops.attn_mem_bwd(d["mem"], d["bv"], f["probs"], f["psum"], o["qk"], o["dmbar"], d["dctx"], B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=SITE, rng=rng,
                     dmem=b["dmem"], out=(b["dsc"], b["dqk"], b["dcp"], b["dbv"]))
    launch(ops, [head_reduce_job(b["dqk"], d["Wk"], o["dq"], B, H, dh), head_wgrad_job(d["q"], b["dqk"], o["dWk"], B, H, dh),
                 head_wgrad_job(d["dctx"], f["mbar"], o["dWv"], B, H, dh)])
    for g in (o, f, b):
        g.check()
    got = dict(ctx=ctx, dq=o["dq"], dWk=o["dWk"], dWv=o["dWv"], dbv=b["dbv"], dmem=b["dmem"])
    errs = {n: note("block", (shape, p), n, err(t, std[n]), TOL_BLOCK) for n, t in got.items()}
    for n, e in errs.items():
        assert e < TOL_BLOCK, (n, e)
