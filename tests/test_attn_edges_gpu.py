"""GPU: encoder self-attention as the plans call it (csrc/tf_plan.hip: fp32 output NULL, the result only as bf16 hi / lo planes
stored by store_rows_via_lds or, where planes_rows_ok is false, by the per-element fallback), at the edges of the one-tile
kernels.  Cases, reference and yardsticks live in tests/attention_ref.py; tests/test_attention_ref_cpu.py judges them.

  a. the fp32 outputs against fp64 per (batch, head) block: bound = 4 x (e_fmt + e_fp32) of that tensor and case, floored at 2e-5
     (the rule of tests/test_rnn_kernels_gpu.py, computed at run time; nothing hard-coded here);
  b. every output pre-filled with a sentinel: none left inside, nothing touched outside (the plans rely on the zero padding of
     plane rows >= S*B surviving the producer);
  c. planes == split of the fp32 twin, bit for bit, for fp32 + planes and for planes alone, forward and backward; the
     wave-per-row kernels (S > 64) and the cross backward likewise;
  d. the element fallbacks (unaligned planes, a q8 plane) give the bits of the row pieces;
  e. a fully masked query row is NaN in both planes;
  f. the buffer a Transformer plan's out-projection reads (enc0.ctxp) is that result.

SLNLP_ATTN_EDGES_PROFILE=<path>: also write the measured errors and their bounds per case there
(profiles/attn_edges_parity.json)."""
import json
import math
import os

import pytest
import torch

import attention_ref as ar
import kernel_refs as kr
from kernel_refs import planes_are_the_split_of
from test_kernels_gpu import _e4m3_decode

pytestmark = pytest.mark.gpu

PAD, SITE = ar.PAD, ar.DROP_SITE
P_DROP = 0.2
F32_SENTINEL = -1.2345678e30       # finite, and no result of these inputs
W16_SENTINEL = 0x7FA5              # a bf16 NaN with a payload: no split of a number is a NaN, and the NaN the hardware makes is quiet 0x7FC0 / 0xFFC0
SELF_CASES = ([(c, True, True) for c in ar.SELF_EDGE] + ar.SELF_VARIANTS)
MEASURED = {}


def _id(v):
    case, causal, use_ids = v
    return ar.case_id(case) + ("" if causal and use_ids else f"-causal{int(causal)}-ids{int(use_ids)}")


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    yield o
    path = os.environ.get("SLNLP_ATTN_EDGES_PROFILE")
    if path and MEASURED:
        doc = {"what": "tests/test_attn_edges_gpu.py on an MI355X: block_err (max |kernel - fp64 reference| per (batch, head) block over that "
                       "block's max |reference|, the worst block) of the fp32 outputs of slnlp_attn_self_fwd_ex / _bwd_ex, and the bound "
                       "4 x (e_fmt + e_fp32) floored at 2e-5 it was held to; case = B-S-H-dh[-causal-ids] p",
               "cases": dict(sorted(MEASURED.items()))}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


# ------------------------------------------------------------------------------------------------ buffers with sentinels
def _alloc_rows(M):
    from slnlp.ops import pad64
    return pad64(M) + 64


def _f32_buf(M, W):
    return torch.full((_alloc_rows(M), W), F32_SENTINEL, dtype=torch.float32, device="cuda")


def _plane_buf(M, W, offset=0):
    """A sentinel-filled [rows, W] int16 buffer whose first element sits ``offset`` elements behind a fresh allocation."""
    n = _alloc_rows(M) * W
    flat = torch.full((n + offset,), W16_SENTINEL, dtype=torch.int16, device="cuda")
    return flat, flat[offset:].view(_alloc_rows(M), W)


def _outputs(M, W, mode, key, offset=0):
    """(out dict for ops.attn_*_ex, everything allocated) for mode "fp32" / "both" / "planes"."""
    out, held = {}, {}
    if mode != "planes":
        held[key] = _f32_buf(M, W)
        out[key] = held[key][:M]
    if mode != "fp32":
        (fh, hi), (fl, lo) = _plane_buf(M, W, offset), _plane_buf(M, W, offset)
        held["planes"], held["flat"] = (hi, lo), (fh, fl)
        out["planes"] = (hi[:M], lo[:M])
    return out, held


def _written_and_nothing_else(held, M, key, offset=0):
    """(b): no sentinel left in rows < M, every word beyond still the sentinel."""
    if key in held:
        buf = held[key].cpu()
        assert bool((buf[:M] != F32_SENTINEL).all()), f"{key}: an element was not written"
        assert bool((buf[M:] == F32_SENTINEL).all()), f"{key}: written past its rows"
    for name, p, flat in zip(("hi", "lo"), held.get("planes", ()), held.get("flat", ())):
        p, s = p.cpu(), W16_SENTINEL
        assert bool((p[:M] != s).all()), f"{key} {name} plane: an element was not written"
        assert bool((p[M:] == s).all()), f"{key} {name} plane: written past its rows"
        assert bool((flat[:offset].cpu() == s).all()), f"{key} {name} plane: written before its first element"


# ------------------------------------------------------------------------------------------------ one case, every call of it
_RUNS = {}


def _self_calls(ops, dev, B, S, H, dh, causal, p, rng, modes, offset=0, ids_dev=None):
    """Forward and backward through the _ex launchers once per mode, every output pre-filled -> {mode: dict}."""
    E, M = H * dh, S * B
    res = {}
    for mode in modes:
        of, hf = _outputs(M, E, mode, "ctx", offset)
        f = ops.attn_self_fwd_ex(dev["qkv"], ids_dev, PAD, B=B, S=S, H=H, dh=dh, causal=causal, drop_p=p, drop_site=SITE, rng=rng,
                                 planes_only=mode == "planes", out=of)
        assert (f["ctx"] is None) == (mode == "planes")
        ob, hb = _outputs(M, 3 * E, mode, "dqkv", offset)
        g = ops.attn_self_bwd_ex(dev["qkv"], f["probs"], dev["dctx"], B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=SITE, rng=rng,
                                 planes_only=mode == "planes", out=ob)
        assert (g["dqkv"] is None) == (mode == "planes")
        torch.cuda.synchronize()
        res[mode] = dict(fwd=hf, bwd=hb, probs=f["probs"].cpu(),
                         ctx=None if f["ctx"] is None else f["ctx"].cpu(), dqkv=None if g["dqkv"] is None else g["dqkv"].cpu(),
                         ctx_planes=tuple(t.cpu() for t in f["planes"]) if f["planes"] else None,
                         dqkv_planes=tuple(t.cpu() for t in g["planes"]) if g["planes"] else None)
    return res


def run_case(ops, case, causal=True, use_ids=True, p=0.0):
    """Inputs, dropout mask, fp64 reference with its yardsticks, and the three calls of (c) -- computed once per case and shared
    by the tests below, which leave it unchanged."""
    key = (case, causal, use_ids, p)
    if key not in _RUNS:
        B, S, H, dh = case
        inp = ar.self_inputs(B, S, H, dh, use_ids)
        rng = ops.make_rng(seed=5, step=2)
        mask = ops.dropout_mask(B * H * S, S, p, SITE, rng).cpu().double().view(B, H, S, S) if p > 0 else None
        ref, e_fp32, e_fmt = ar.attn_yardsticks(inp, B, S, H, dh, causal, mask, p)
        dev = dict(qkv=inp["qkv"].cuda(), dctx=inp["dctx"].cuda())
        ids_dev = inp["ids"].cuda() if use_ids else None
        modes = ("fp32", "both", "planes") if S <= 64 else ("fp32", "both")
        _RUNS[key] = dict(inp=inp, dev=dev, ids_dev=ids_dev, rng=rng, ref=ref, e_fp32=e_fp32, e_fmt=e_fmt,
                          calls=_self_calls(ops, dev, B, S, H, dh, causal, p, rng, modes, ids_dev=ids_dev))
    return _RUNS[key]


def _held(tag, got, run, B, H):
    """Measure, print, record, then assert (a)'s bound for every tensor of ``got``."""
    errs = ar.errors(got, run["ref"], B, H)
    rec, failed = {}, []
    for k, e in errs.items():
        bound = ar.bound(run["e_fmt"][k], run["e_fp32"][k])
        print(f"{tag} {k}: err {e:.2e} e_fmt {run['e_fmt'][k]:.2e} e_fp32 {run['e_fp32'][k]:.2e} bound {bound:.2e}")
        rec[k] = {"err": float(f"{e:.3e}"), "bound": float(f"{bound:.3e}")}
        if not e < bound:
            failed.append((k, e, bound))
    MEASURED[tag] = rec
    assert not failed, (tag, failed)


# ============================================================================================================ a. fp32 against fp64
@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("case,causal,use_ids", [pytest.param(*v, id=_id(v)) for v in SELF_CASES])
def test_fp32_outputs_per_block_against_fp64(ops, case, causal, use_ids, p):
    B, S, H, dh = case
    run = run_case(ops, case, causal, use_ids, p)
    for k in ("probs", "ctx", "dqkv"):
        assert not torch.isnan(run["ref"][k]).any()
        assert run["e_fp32"][k] <= ar.COND, (k, run["e_fp32"][k])          # the premise of the bound (test_attention_ref_cpu.py)
    c = run["calls"]["fp32"]
    _held(f"{_id((case, causal, use_ids))} p{p}", dict(probs=c["probs"], ctx=c["ctx"], dqkv=c["dqkv"]), run, B, H)


def test_ids_with_a_row_stride_other_than_S(ops):
    """ids as a view of a [B, S + 3] matrix whose padding columns hold the pad id: a kernel that indexed with S would mask the
    wrong keys.  Same bits as the contiguous ids."""
    case = (3, 20, 2, 24)
    B, S, H, dh = case
    run = run_case(ops, case, True, True, 0.0)
    ids = run["inp"]["ids"]
    wide = torch.full((B, S + 3), PAD, dtype=torch.long)
    wide[:, :S] = ids
    assert not torch.equal(wide.flatten()[:B * S].view(B, S), ids)         # read with stride S these are other ids
    view = wide.cuda()[:, :S]
    assert view.stride(0) == S + 3
    f = ops.attn_self_fwd_ex(run["dev"]["qkv"], view, PAD, B=B, S=S, H=H, dh=dh, causal=True, want_planes=True)
    c = run["calls"]["both"]
    assert torch.equal(f["probs"].cpu(), c["probs"]) and torch.equal(f["ctx"].cpu(), c["ctx"])
    assert planes_are_the_split_of(f["planes"], f["ctx"])
    e = ar.block_err(f["probs"], run["ref"]["probs"])
    assert e < ar.bound(run["e_fmt"]["probs"], run["e_fp32"]["probs"]), e


# ============================================================================================================ b. written, and nothing else
@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("case,causal,use_ids", [pytest.param(*v, id=_id(v)) for v in SELF_CASES] +
                         [pytest.param(c, True, True, id=ar.case_id(c)) for c in ar.LONG_PLANES])
def test_every_element_written_and_nothing_else(ops, case, causal, use_ids, p):
    B, S, H, dh = case
    run = run_case(ops, case, causal, use_ids, p)
    for mode, c in run["calls"].items():
        _written_and_nothing_else(c["fwd"], S * B, "ctx")
        _written_and_nothing_else(c["bwd"], S * B, "dqkv")


# ============================================================================================================ c. planes == split of fp32
@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("case,causal,use_ids", [pytest.param(*v, id=_id(v)) for v in SELF_CASES] +
                         [pytest.param(c, True, True, id=ar.case_id(c)) for c in ar.LONG_PLANES])
def test_planes_are_the_split_of_the_fp32_result(ops, case, causal, use_ids, p):
    """fp32 only / fp32 + planes / planes only (the plans' call; S <= 64) on the same inputs and rng.  The same accumulators feed
    the fp32 store, the element store and the row pieces, and all split with split_bf16: no tolerance."""
    B, S, H, dh = case
    calls = run_case(ops, case, causal, use_ids, p)["calls"]
    one, two = calls["fp32"], calls["both"]
    for k in ("probs", "ctx", "dqkv"):
        assert torch.equal(one[k], two[k]), f"{k}: the fp32 output changes when planes are asked for"
    for k in ("ctx", "dqkv"):
        assert planes_are_the_split_of(two[k + "_planes"], two[k]), f"{k}: fp32 + planes"
    if S <= 64:
        three = calls["planes"]
        assert torch.equal(one["probs"], three["probs"])
        for k in ("ctx", "dqkv"):
            assert planes_are_the_split_of(three[k + "_planes"], one[k]), f"{k}: planes only (fp32 output NULL)"


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("case", ar.CROSS_PLANES, ids=ar.case_id)
def test_cross_backward_planes_are_the_split_of_dkv(ops, case, p):
    """attn_cross_bwd's PlaneOut (no caller in either plan today) through slnlp_attn_cross_bwd_ex, kv and dkv as column views
    of buffers 8 floats wider: dq / dkv keep their bits, the planes are the split of dkv, the padding columns and rows stay."""
    B, S, H, dh = case
    E, M, ld = H * dh, S * B, 2 * H * dh + ar.CROSS_LD_PAD
    inp = ar.cross_inputs(B, S, H, dh)
    q, kv, dctx = inp["q"].cuda(), inp["kv_wide"].cuda()[:, :2 * E], inp["dctx"].cuda()
    assert kv.stride(0) == ld
    rng = ops.make_rng(seed=8, step=1)
    ctx, probs = ops.attn_cross_fwd(q, kv, B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=9, rng=rng)
    got = {}
    for mode in ("fp32", "both"):
        wide = _f32_buf(M, ld)
        out = dict(dkv=wide[:M, :2 * E])
        if mode == "both":
            (_, hi), (_, lo) = _plane_buf(M, ld), _plane_buf(M, ld)
            out["planes"] = (hi[:M, :2 * E], lo[:M, :2 * E])
        r = ops.attn_cross_bwd_ex(q, kv, probs, dctx, B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=9, rng=rng, out=out)
        torch.cuda.synchronize()
        w = wide.cpu()
        assert bool((w[:M, :2 * E] != F32_SENTINEL).all()) and bool((w[:M, 2 * E:] == F32_SENTINEL).all()) and bool((w[M:] == F32_SENTINEL).all())
        got[mode] = dict(dq=r["dq"].cpu(), dkv=r["dkv"].cpu())
        if mode == "both":
            s = W16_SENTINEL
            for t in (hi.cpu(), lo.cpu()):
                assert bool((t[:M, :2 * E] != s).all()) and bool((t[:M, 2 * E:] == s).all()) and bool((t[M:] == s).all())
            assert planes_are_the_split_of(r["planes"], r["dkv"])
    dq0, dkv0 = ops.attn_cross_bwd(q, kv, probs, dctx, B=B, S=S, H=H, dh=dh, drop_p=p, drop_site=9, rng=rng)
    for g in got.values():
        assert torch.equal(g["dq"], dq0.cpu()) and torch.equal(g["dkv"], dkv0.cpu())


# ============================================================================================================ d. the fallbacks
@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("case", [(3, 20, 2, 24), (2, 19, 1, 192)], ids=ar.case_id)
def test_unaligned_planes_take_the_element_path_with_the_same_bits(ops, case, p):
    """Planes only, the plane pointers 4 elements (8 bytes) past a 16-byte boundary: a valid call, planes_rows_ok is false, the
    element stores run with no fp32 output.  The planes equal those of the aligned call (row pieces)."""
    B, S, H, dh = case
    run = run_case(ops, case, True, True, p)
    off = _self_calls(ops, run["dev"], B, S, H, dh, True, p, run["rng"], ("planes",), offset=4, ids_dev=run["ids_dev"])["planes"]
    for t in off["fwd"]["planes"] + off["bwd"]["planes"]:
        assert t.data_ptr() % 16 == 8
    for t in run["calls"]["planes"]["fwd"]["planes"]:
        assert t.data_ptr() % 16 == 0
    _written_and_nothing_else(off["fwd"], S * B, "ctx", offset=4)
    _written_and_nothing_else(off["bwd"], S * B, "dqkv", offset=4)
    aligned = run["calls"]["planes"]
    assert torch.equal(off["probs"], aligned["probs"])
    for k in ("ctx_planes", "dqkv_planes"):
        for a, b in zip(off[k], aligned[k]):
            assert torch.equal(a, b), f"{k}: element path and row pieces differ"


@pytest.mark.parametrize("planes_only", [False, True], ids=["with-ctx", "planes-only"])
def test_q8_plane_is_the_nearest_e4m3_and_leaves_the_planes_alone(ops, planes_only):
    case = (3, 20, 2, 24)
    B, S, H, dh = case
    E, M = H * dh, S * B
    run = run_case(ops, case, True, True, 0.0)
    of, hf = _outputs(M, E, "planes" if planes_only else "both", "ctx")
    q8buf = torch.full((_alloc_rows(M), E), 0x7F, dtype=torch.uint8, device="cuda")          # e4m3 NaN: no clamped number encodes to it
    of["q8"] = q8buf[:M]
    f = ops.attn_self_fwd_ex(run["dev"]["qkv"], run["ids_dev"], PAD, B=B, S=S, H=H, dh=dh, causal=True, planes_only=planes_only, out=of)
    torch.cuda.synchronize()
    _written_and_nothing_else(hf, M, "ctx")
    both = run["calls"]["both"]
    for a, b in zip(f["planes"], both["ctx_planes"]):
        assert torch.equal(a.cpu(), b)
    if not planes_only:
        assert torch.equal(f["ctx"].cpu(), both["ctx"])
    q = q8buf.cpu()
    assert bool((q[M:] == 0x7F).all()) and bool((q[:M] != 0x7F).all())
    v = both["ctx"].double().clamp(-448.0, 448.0)
    d = (_e4m3_decode(q[:M]) - v).abs()
    normal = v.abs() >= 2.0 ** -6
    assert bool(normal.any()) and bool((~normal).any())                   # both branches of the bound are exercised
    assert bool((d[normal] <= 2.0 ** -4 * v.abs()[normal]).all())          # half an ulp of three mantissa bits
    assert bool((d[~normal] <= 2.0 ** -10).all())                         # half the subnormal spacing 2^-9


# ============================================================================================================ e. a fully masked row
def test_fully_masked_row_is_nan_in_both_planes(ops):
    """The shape of test_kernels_gpu.py::test_attn_self_fully_masked_row_is_nan: sequence 1's first key is <pad>, so its query 0
    sees no key.  That row's planes are NaN in both words (by value, not by bit pattern); every other row is the split."""
    B, S, H, dh = 2, 8, 2, 8
    E, M = H * dh, S * B
    qkv = ar.rnd(M, 3 * E, seed=1).cuda()
    ids = torch.full((B, S), ar.REAL, dtype=torch.long)
    ids[1, 0] = PAD
    row = 0 * B + 1
    others = [m for m in range(M) if m != row]
    ctx = None
    for mode in ("both", "planes"):
        of, hf = _outputs(M, E, mode, "ctx")
        f = ops.attn_self_fwd_ex(qkv, ids.cuda(), PAD, B=B, S=S, H=H, dh=dh, causal=True, planes_only=mode == "planes", out=of)
        torch.cuda.synchronize()
        assert torch.isnan(f["probs"][1, :, 0]).all() and not torch.isnan(f["probs"][0]).any()
        if mode == "both":
            ctx = f["ctx"].cpu()
            assert bool(torch.isnan(ctx[row]).all()) and not bool(torch.isnan(ctx[others]).any())
        hi, lo = [t.cpu() for t in f["planes"]]
        for t, full in zip((hi, lo), hf["planes"]):
            dec = t.view(torch.bfloat16).float()
            assert bool(torch.isnan(dec[row]).all()), f"{mode}: the masked row is not NaN in a plane"
            assert not bool(torch.isnan(dec[others]).any()), f"{mode}: a NaN outside the masked row"
            assert bool((full.cpu()[M:] == W16_SENTINEL).all())
        assert planes_are_the_split_of((hi[others], lo[others]), ctx[others]), mode


# ============================================================================================================ f. the plan takes this path
def test_plan_ctx_planes_are_the_reference_on_the_plans_own_inputs():
    """One small Transformer engine (E = 64, F = 64: the plane path; S = 20 <= 64: ctx leaves the kernel as planes only), eval
    forward.  ctx rebuilt in fp64 from the tapped embedding and the engine's in_proj weight and bias; hi + lo of the tapped
    enc0.ctxp -- what the out-projection GEMM reads -- against it per block, bound 4 x (e_fmt + e_fp32) floored at 2e-5 with the
    in-projection inside both yardsticks.  (Layer 0's in_proj weight is scaled down first, see below: on the unscaled synthetic
    weights float32 itself misses the premise of that bound.)"""
    from oracle import transformer_ref as tr
    from slnlp import synth, tf_engine as te
    E, F, N, S, B, H, Vs, Vt = 64, 64, 1, 20, 3, 2, 64, 16
    dh, M = E // H, S * B
    cfg = te.make_config(E, H, N, F, Vs, Vt, B, S)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_weights(tr.param_shapes(E, H, N, F, Vs, Vt), seed=1).items()}
    # The embedding is the table row times sqrt(E) = 8 plus the position: through synth's in_proj weights that gives |qkv| ~ 20 and
    # scores of several hundred, where torch float32 itself is 5e-6 from fp64 on ctx (softmax of x moves by |x| ulps) and no bound
    # of a few x e_fmt says anything about a kernel.  The in-projection weight is divided by sqrt(E), which puts |qkv| at ~ 3 as in
    # the kernel cases above; the premise (e_fp32 <= COND) is asserted below either way.
    pre = "transformer.encoder.layers.0.self_attn."
    sd[pre + "in_proj_weight"] = sd[pre + "in_proj_weight"] / math.sqrt(E)
    Xn, _, yn = synth.make_batch(B, S, Vs, Vt, seed=1, min_len=3)
    X, y = torch.from_numpy(Xn), torch.from_numpy(yn)
    eng = te.TransformerEngine(cfg, device="cuda:0")
    eng.load_state(sd)
    eng.forward(X.cuda(), y.cuda(), train=False)
    torch.cuda.synchronize()
    x0 = eng.tap("src_embed", M, E).cpu()
    w = eng.tap("enc0.ctxp", M, E).view(torch.int16).view(2, M, E).cpu()
    W, bias = sd[pre + "in_proj_weight"], sd[pre + "in_proj_bias"]

    def rebuild(dtype, product):
        qkv = product(x0.to(dtype), W.to(dtype).T) + bias.to(dtype)
        return ar.mha_ref(qkv, X, cfg.pad_src, B, S, H, dh, True, product=product)[0].double()

    ref = rebuild(torch.float64, torch.matmul)
    assert not torch.isnan(ref).any()
    e_fp32 = ar.block_err(rebuild(torch.float32, torch.matmul), ref, B, H)
    e_fmt = ar.block_err(rebuild(torch.float64, lambda a, b: kr.fmt_matmul(a, b, 3)), ref, B, H)
    assert e_fp32 <= ar.COND, e_fp32                     # these are the engine's embeddings, not a case judged on the CPU
    e, bound = ar.block_err(ar.planes_value((w[0], w[1])), ref, B, H), ar.bound(e_fmt, e_fp32)
    print(f"plan enc0.ctxp: err {e:.2e} e_fmt {e_fmt:.2e} e_fp32 {e_fp32:.2e} bound {bound:.2e}")
    MEASURED["plan enc0.ctxp (E64 F64 N1 S20 B3 H2, eval)"] = {"ctx": {"err": float(f"{e:.3e}"), "bound": float(f"{bound:.3e}")}}
    assert e < bound, (e, bound)
