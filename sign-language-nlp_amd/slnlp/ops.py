"""Thin torch-tensor front-ends of the granular C-ABI kernels (used by the
parity tests and by the RNN host code).  Every function launches on torch's
current stream and fails loudly without a GPU / without the built library."""
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import _lib, _packed
from ._lib import GemmArgs, check, load, ptr, stream_ptr


def make_rng(seed=0, step=0, device="cuda"):
    """Dropout state {seed, step} as int64[2] on the device (read as uint64)."""
    return torch.tensor([seed, step], dtype=torch.int64, device=device)


def gemm(A, B, *, M, N, K, a_kmajor=True, b_kmajor=True, lda=None, ldb=None, out=None, ldc=None,
         bias=None, relu=False, gate=None, gate_scale=1.0, gate_mode=0, drop_p=0.0, drop_site=0, rng=None,
         resid=None, rowsum_a=None, precision=3):
    _lib.require_gpu()
    lda = lda if lda is not None else (K if a_kmajor else M)
    ldb = ldb if ldb is not None else (K if b_kmajor else N)
    ldc = ldc if ldc is not None else N
    if out is None:
        out = torch.empty(M, ldc, dtype=torch.float32, device=A.device)
    a = GemmArgs()
    a.A, a.lda, a.a_kmajor = ptr(A), lda, int(a_kmajor)
    a.B, a.ldb, a.b_kmajor = ptr(B), ldb, int(b_kmajor)
    a.C, a.ldc, a.M, a.N, a.K = ptr(out), ldc, M, N, K
    a.bias, a.relu = ptr(bias), int(relu)
    a.gate, a.ldg, a.gate_scale = ptr(gate), (gate.stride(0) if gate is not None else 0), gate_scale
    a.drop_p, a.drop_site, a.rng = drop_p, drop_site, ptr(rng)
    a.resid, a.ldr = ptr(resid), (resid.stride(0) if resid is not None else 0)
    a.rowsum_a, a.precision, a.gate_mode = ptr(rowsum_a), precision, gate_mode
    check(load().slnlp_gemm(C.byref(a), stream_ptr()), "gemm")
    return out


def pad64(n):
    return (n + 63) // 64 * 64


def split_planes(x, want_lo=True):
    """fp32 [R,C] -> (hi, lo) bf16 planes (int16 storage) zero-padded to multiples of 64."""
    _lib.require_gpu()
    R, Cc = x.shape
    hi = torch.zeros(pad64(R), pad64(Cc), dtype=torch.int16, device=x.device)
    lo = torch.zeros_like(hi) if want_lo else None
    check(load().slnlp_split_planes(ptr(x), x.stride(0), R, Cc, ptr(hi), ptr(lo), hi.stride(0), stream_ptr()), "split_planes")
    return hi, lo


def pad128(n):
    return (n + 127) // 128 * 128


def quant_rows_fp8(x):
    """fp32 [R,K] -> (q uint8 [pad64(R), pad128(K)] OCP e4m3, scale fp32 [R]): q[r] = e4m3(x[r] / scale[r]), scale[r] = max|x[r]| / 448."""
    _lib.require_gpu()
    R, K = x.shape
    q = torch.zeros(pad64(R), pad128(K), dtype=torch.uint8, device=x.device)
    scale = torch.empty(R, dtype=torch.float32, device=x.device)
    check(load().slnlp_quant_rows_fp8(ptr(x), x.stride(0), R, K, ptr(q), q.stride(0), ptr(scale), stream_ptr()), "quant_rows_fp8")
    return q, scale


def gemm_fp8(Aq, Bq, *, M, N, K, col_scale=None, bias=None, relu=False, resid=None, out=None, want_q8=False):
    """C = (A8 B8^T) * col_scale (+ bias, relu, resid) over e4m3 byte planes (both k-major) on the fp8 MFMA (precision 8)."""
    _lib.require_gpu()
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=Aq.device)
    a = GemmArgs()
    a.C, a.ldc, a.M, a.N, a.K = ptr(out), out.stride(0), M, N, K
    a.a_kmajor, a.b_kmajor, a.precision = 1, 1, 8
    a.A_hi, a.lda_p, a.B_hi, a.ldb_p = ptr(Aq), Aq.stride(0), ptr(Bq), Bq.stride(0)
    a.col_scale, a.bias, a.relu = ptr(col_scale), ptr(bias), int(relu)
    a.resid, a.ldr = ptr(resid), (resid.stride(0) if resid is not None else 0)
    cq = None
    if want_q8:
        cq = torch.zeros(pad64(M), pad128(N), dtype=torch.uint8, device=out.device)
        a.C_q8, a.ldc_p = ptr(cq), cq.stride(0)
    check(load().slnlp_gemm(C.byref(a), stream_ptr()), "gemm_fp8")
    return (out, cq) if want_q8 else out


def plane_job(Ap, Bp, *, M, N, K, a_kmajor=True, b_kmajor=True, out=None, precision=3, rowsum_a=None, bias=None,
              relu=False, resid=None):
    """GemmArgs of one pre-split GEMM (for gemm_group); returns (args, out)."""
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=Ap[0].device)
    a = GemmArgs()
    a.C, a.ldc, a.M, a.N, a.K = ptr(out), out.stride(0), M, N, K
    a.a_kmajor, a.b_kmajor, a.precision = int(a_kmajor), int(b_kmajor), precision
    a.A_hi, a.A_lo, a.lda_p = ptr(Ap[0]), ptr(Ap[1]), Ap[0].stride(0)
    a.B_hi, a.B_lo, a.ldb_p = ptr(Bp[0]), ptr(Bp[1]), Bp[0].stride(0)
    a.bias, a.relu, a.rowsum_a = ptr(bias), int(relu), ptr(rowsum_a)
    a.resid, a.ldr = ptr(resid), (resid.stride(0) if resid is not None else 0)
    return a, out


def gemm_group(jobs, split_k=None, scratch=None):
    """ONE launch for up to 4 plane GEMMs (list of GemmArgs); split_k[i] > 1 = deterministic split-K."""
    _lib.require_gpu()
    n = len(jobs)
    arr = (GemmArgs * n)(*jobs)
    sk = (C.c_int32 * n)(*(split_k or [1] * n))
    if scratch is None:
        nbytes = int(load().slnlp_gemm_group_scratch_bytes(arr, sk, n))
        scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    check(load().slnlp_gemm_group(arr, sk, n, ptr(scratch), scratch.numel(), stream_ptr()), "gemm_group")
    return scratch


def plane_geo(jobs, split_k=None):
    """Tile geometry (0 .. 4: 64x64, 128x128 64-k, 128x128 32-k, 256x256 32-k, 96x64) a launch of these plane jobs takes; no device."""
    n = len(jobs)
    arr = (GemmArgs * n)(*jobs)
    sk = (C.c_int32 * n)(*(split_k or [1] * n))
    return int(load().slnlp_plane_geo(arr, sk, n))


def gemm_wd_plan(jw, jd):
    """(split, separate, geometry of the wgrad launch, of the dgrad launch) the library picks for this gradient pair."""
    v = [C.c_int32(0) for _ in range(4)]
    check(load().slnlp_gemm_wd_plan(C.byref(jw), C.byref(jd), *[C.byref(x) for x in v]), "gemm_wd_plan")
    return tuple(int(x.value) for x in v)


def gemm_wd(jw, jd, scratch=None):
    """The gradient pair of one dY (plane_job wgrad + dgrad) launched as the training plans launch it (slnlp_gemm_wd)."""
    _lib.require_gpu()
    if scratch is None:
        arr = (GemmArgs * 2)(jw, jd)
        sk = (C.c_int32 * 2)(8, 1)
        scratch = torch.zeros(int(load().slnlp_gemm_group_scratch_bytes(arr, sk, 2)), dtype=torch.uint8, device="cuda")
    check(load().slnlp_gemm_wd(C.byref(jw), C.byref(jd), ptr(scratch), scratch.numel(), stream_ptr()), "gemm_wd")
    return scratch


def gemm_planes(Ap, Bp, *, M, N, K, a_kmajor=True, b_kmajor=True, out=None, precision=3, rowsum_a=None, bias=None,
                relu=False, resid=None, want_planes=False):
    """C = A B^T over pre-split operands Ap = (hi, lo), Bp = (hi, lo) (see split_planes)."""
    _lib.require_gpu()
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=Ap[0].device)
    a = GemmArgs()
    a.C, a.ldc, a.M, a.N, a.K = ptr(out), out.stride(0), M, N, K
    a.a_kmajor, a.b_kmajor, a.precision = int(a_kmajor), int(b_kmajor), precision
    a.A_hi, a.A_lo, a.lda_p = ptr(Ap[0]), ptr(Ap[1]), Ap[0].stride(0)
    a.B_hi, a.B_lo, a.ldb_p = ptr(Bp[0]), ptr(Bp[1]), Bp[0].stride(0)
    a.bias, a.relu, a.rowsum_a = ptr(bias), int(relu), ptr(rowsum_a)
    a.resid, a.ldr = ptr(resid), (resid.stride(0) if resid is not None else 0)
    cp = None
    if want_planes:
        cp = (torch.zeros(pad64(M), pad64(N), dtype=torch.int16, device=out.device),
              torch.zeros(pad64(M), pad64(N), dtype=torch.int16, device=out.device))
        a.C_hi, a.C_lo, a.ldc_p = ptr(cp[0]), ptr(cp[1]), cp[0].stride(0)
    check(load().slnlp_gemm(C.byref(a), stream_ptr()), "gemm_planes")
    return (out, cp) if want_planes else out


def gemm_rows(Ap, W, *, M, N, K, out=None, precision=3, bias=None, relu=0, gate=None, gate_scale=1.0, gate_mode=0, drop_p=0.0,
              drop_site=0, rng=None, drop_head_dim=0, resid=None, want_planes=False):
    """C = A W^T for a few rows (the decoder's products): A as k-major planes Ap = (hi, lo), the weight W [N, K] as fp32 (the kernel
    splits it in registers -- the same bits as split_planes(W)): slnlp_gemm_rows."""
    _lib.require_gpu()
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=Ap[0].device)
    a = GemmArgs()
    a.C, a.ldc, a.M, a.N, a.K = ptr(out), out.stride(0), M, N, K
    a.a_kmajor, a.b_kmajor, a.precision = 1, 1, precision
    a.A_hi, a.A_lo, a.lda_p = ptr(Ap[0]), ptr(Ap[1]), Ap[0].stride(0)
    a.B, a.ldb = ptr(W), W.stride(0)
    a.bias, a.relu = ptr(bias), int(relu)
    a.gate, a.ldg, a.gate_scale, a.gate_mode = ptr(gate), (gate.stride(0) if gate is not None else 0), gate_scale, gate_mode
    a.drop_p, a.drop_site, a.rng, a.drop_head_dim = drop_p, drop_site, ptr(rng), drop_head_dim
    a.resid, a.ldr = ptr(resid), (resid.stride(0) if resid is not None else 0)
    cp = None
    if want_planes:
        cp = (torch.zeros(pad64(M), pad64(N), dtype=torch.int16, device=out.device),
              torch.zeros(pad64(M), pad64(N), dtype=torch.int16, device=out.device))
        a.C_hi, a.C_lo, a.ldc_p = ptr(cp[0]), ptr(cp[1]), cp[0].stride(0)
    check(load().slnlp_gemm_rows(C.byref(a), stream_ptr()), "gemm_rows")
    return (out, cp) if want_planes else out


def gemm_rows_ln(x, gamma, beta, W, *, M, N, K, y, stats=None, y_planes=None, eps=1e-5, out=None, precision=3, bias=None, relu=0,
                 drop_p=0.0, drop_site=0, rng=None, drop_head_dim=0, resid=None, out_planes=None):
    """C = epilogue(LayerNorm(x) W^T) in one launch (slnlp_gemm_rows_ln): x [M, K] fp32 is the LayerNorm's input; the normalised
    rows go to ``y`` [M, K], (mean, rstd) to ``stats`` [M, 2] and, as (hi, lo) planes, to ``y_planes`` -- what layernorm_fwd
    followed by gemm_rows would have left, bit for bit.  ``out_planes``: also emit C as (hi, lo) planes."""
    _lib.require_gpu()
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    a = GemmArgs()
    a.C, a.ldc, a.M, a.N, a.K = ptr(out), out.stride(0), M, N, K
    a.a_kmajor, a.b_kmajor, a.precision = 1, 1, precision
    a.B, a.ldb = ptr(W), W.stride(0)
    a.bias, a.relu = ptr(bias), int(relu)
    a.drop_p, a.drop_site, a.rng, a.drop_head_dim = drop_p, drop_site, ptr(rng), drop_head_dim
    a.resid, a.ldr = ptr(resid), (resid.stride(0) if resid is not None else 0)
    if out_planes is not None:
        a.C_hi, a.C_lo, a.ldc_p = ptr(out_planes[0]), ptr(out_planes[1]), out_planes[0].stride(0)
    yh, yl = y_planes if y_planes is not None else (None, None)
    check(load().slnlp_gemm_rows_ln(C.byref(a), ptr(x), x.stride(0), ptr(gamma), ptr(beta), eps, ptr(y), ptr(stats), ptr(yh), ptr(yl),
                                    yh.stride(0) if yh is not None else 0, stream_ptr()), "gemm_rows_ln")
    return out


def gemm_rows_bwd(dYp, W, Xp, *, B, Nout, Kin, precision=3, gate=None, gate_scale=1.0, gate_mode=0, drop_p=0.0, drop_site=0, rng=None,
                  drop_head_dim=0, resid=None, want_planes=False, want_db=True):
    """dX = dY W (+ epilogue), dW = dY^T x, db = colsum(dY) in one launch (slnlp_gemm_rows_bwd): dYp [B, Nout] and Xp [B, Kin] as
    (hi, lo) planes, the weight W [Nout, Kin] as fp32."""
    _lib.require_gpu()
    dev = dYp[0].device
    dX = torch.empty(B, Kin, dtype=torch.float32, device=dev)
    dW = torch.empty(Nout, Kin, dtype=torch.float32, device=dev)
    db = torch.empty(Nout, dtype=torch.float32, device=dev) if want_db else None
    d, w = GemmArgs(), GemmArgs()
    d.C, d.ldc, d.M, d.N, d.K = ptr(dX), dX.stride(0), B, Kin, Nout
    d.a_kmajor, d.b_kmajor, d.precision = 1, 0, precision
    d.A_hi, d.A_lo, d.lda_p = ptr(dYp[0]), ptr(dYp[1]), dYp[0].stride(0)
    d.B, d.ldb = ptr(W), W.stride(0)
    d.gate, d.ldg, d.gate_scale, d.gate_mode = ptr(gate), (gate.stride(0) if gate is not None else 0), gate_scale, gate_mode
    d.drop_p, d.drop_site, d.rng, d.drop_head_dim = drop_p, drop_site, ptr(rng), drop_head_dim
    d.resid, d.ldr = ptr(resid), (resid.stride(0) if resid is not None else 0)
    cp = None
    if want_planes:
        cp = (torch.zeros(pad64(B), pad64(Kin), dtype=torch.int16, device=dev), torch.zeros(pad64(B), pad64(Kin), dtype=torch.int16, device=dev))
        d.C_hi, d.C_lo, d.ldc_p = ptr(cp[0]), ptr(cp[1]), cp[0].stride(0)
    w.C, w.ldc, w.M, w.N, w.K = ptr(dW), dW.stride(0), Nout, Kin, B
    w.a_kmajor, w.b_kmajor, w.precision = 0, 0, precision
    w.A_hi, w.A_lo, w.lda_p = ptr(dYp[0]), ptr(dYp[1]), dYp[0].stride(0)
    w.B_hi, w.B_lo, w.ldb_p = ptr(Xp[0]), ptr(Xp[1]), Xp[0].stride(0)
    w.rowsum_a = ptr(db)
    check(load().slnlp_gemm_rows_bwd(C.byref(d), C.byref(w), stream_ptr()), "gemm_rows_bwd")
    return (dX, dW, db, cp) if want_planes else (dX, dW, db)


def embed_fwd(ids, table, pe, *, B, S, scale=None, drop_p=0.0, drop_site=0, rng=None, nan_idx=-1):
    _lib.require_gpu()
    V, E = table.shape
    out = torch.empty(S * B, E, dtype=torch.float32, device=table.device)
    check(load().slnlp_embed_fwd(ptr(ids), ids.stride(0) if ids.ndim == 2 else 1, B, S, E, V, ptr(table), ptr(pe),
                                 ptr(out), float(E ** 0.5 if scale is None else scale), drop_p, drop_site, ptr(rng),
                                 nan_idx, stream_ptr()), "embed_fwd")
    return out


def embed_bwd(ids, dx, *, B, S, V, scale=None, zero_row=-1, drop_p=0.0, drop_site=0, rng=None):
    _lib.require_gpu()
    E = dx.shape[1]
    dt = torch.empty(V, E, dtype=torch.float32, device=dx.device)
    scratch = torch.empty(int(load().slnlp_embed_bwd_scratch_bytes(B, S, E)), dtype=torch.uint8, device=dx.device)
    check(load().slnlp_embed_bwd(ptr(ids), ids.stride(0) if ids.ndim == 2 else 1, B, S, E, V, ptr(dx), ptr(dt),
                                 float(E ** 0.5 if scale is None else scale), zero_row, drop_p, drop_site, ptr(rng),
                                 ptr(scratch), stream_ptr()), "embed_bwd")
    return dt


def _plane_pair(like):
    """Two int16 tensors of ``like``'s shape: the bf16 hi / lo planes a kernel writes beside its fp32 output."""
    return torch.empty_like(like, dtype=torch.int16), torch.empty_like(like, dtype=torch.int16)


def embed_fwd_ex(ids, table, pe, *, B, S, scale=None, drop_p=0.0, drop_site=0, rng=None, nan_idx=-1, want_planes=False,
                 want_keep=False):
    """``embed_fwd`` as the plans call it (``slnlp_embed_fwd_ex``) -> (out, (hi, lo) | None, keep_mask | None): the bf16 planes
    of the output (int16 bit patterns) and, under dropout, the keep bits of each float4 ([S*B*E/4] uint8)."""
    _lib.require_gpu()
    V, E = table.shape
    out = torch.empty(S * B, E, dtype=torch.float32, device=table.device)
    planes = _plane_pair(out) if want_planes else None
    keep = torch.zeros(S * B * E // 4, dtype=torch.uint8, device=table.device) if want_keep else None
    hi, lo = planes if planes else (None, None)
    check(load().slnlp_embed_fwd_ex(ptr(ids), ids.stride(0) if ids.ndim == 2 else 1, B, S, E, V, ptr(table), ptr(pe), ptr(out),
                                    float(E ** 0.5 if scale is None else scale), drop_p, drop_site, ptr(rng), nan_idx, ptr(hi), ptr(lo),
                                    ptr(keep), stream_ptr()), "embed_fwd_ex")
    return out, planes, keep


def embed_bwd_ex(ids, dx, *, B, S, V, scale=None, zero_row=-1, drop_p=0.0, drop_site=0, rng=None, keep_mask=None, out=None):
    """``embed_bwd`` with the keep bits ``embed_fwd_ex`` recorded (``slnlp_embed_bwd_ex``; None: the lots are drawn again) ->
    dtable [V, E], written into ``out`` when given."""
    _lib.require_gpu()
    E = dx.shape[1]
    dt = torch.empty(V, E, dtype=torch.float32, device=dx.device) if out is None else out
    scratch = torch.empty(int(load().slnlp_embed_bwd_scratch_bytes(B, S, E)), dtype=torch.uint8, device=dx.device)
    check(load().slnlp_embed_bwd_ex(ptr(ids), ids.stride(0) if ids.ndim == 2 else 1, B, S, E, V, ptr(dx), ptr(dt),
                                    float(E ** 0.5 if scale is None else scale), zero_row, drop_p, drop_site, ptr(rng), ptr(scratch),
                                    ptr(keep_mask), stream_ptr()), "embed_bwd_ex")
    return dt


def attn_self_fwd(qkv, ids, pad_idx, *, B, S, H, dh, causal=True, drop_p=0.0, drop_site=0, rng=None):
    _lib.require_gpu()
    E = H * dh
    ctx = torch.empty(S * B, E, dtype=torch.float32, device=qkv.device)
    probs = torch.empty(B, H, S, S, dtype=torch.float32, device=qkv.device)
    check(load().slnlp_attn_self_fwd(ptr(qkv), ptr(ids), ids.stride(0) if ids is not None else 0, pad_idx,
                                     int(causal), B, S, H, dh, ptr(ctx), ptr(probs), drop_p, drop_site, ptr(rng),
                                     stream_ptr()), "attn_self_fwd")
    return ctx, probs


def attn_self_bwd(qkv, probs, dctx, *, B, S, H, dh, drop_p=0.0, drop_site=0, rng=None):
    _lib.require_gpu()
    dqkv = torch.empty_like(qkv)
    if S > 64:      # the wave-per-row kernels keep dS between their row pass and their column pass
        scratch = torch.empty(int(load().slnlp_attn_long_scratch_bytes(B, S, H)), dtype=torch.uint8, device=qkv.device)
        check(load().slnlp_attn_self_bwd_long(ptr(qkv), ptr(probs), ptr(dctx), B, S, H, dh, ptr(dqkv), ptr(scratch), drop_p,
                                              drop_site, ptr(rng), stream_ptr()), "attn_self_bwd_long")
        return dqkv
    check(load().slnlp_attn_self_bwd(ptr(qkv), ptr(probs), ptr(dctx), B, S, H, dh, ptr(dqkv), drop_p, drop_site,
                                     ptr(rng), stream_ptr()), "attn_self_bwd")
    return dqkv


def attn_cross_fwd(q, kv, *, B, S, H, dh, drop_p=0.0, drop_site=0, rng=None):
    _lib.require_gpu()
    E = H * dh
    ctx = torch.empty(B, E, dtype=torch.float32, device=q.device)
    probs = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
    check(load().slnlp_attn_cross_fwd(ptr(q), ptr(kv), kv.stride(0), B, S, H, dh, ptr(ctx), ptr(probs), drop_p,
                                      drop_site, ptr(rng), stream_ptr()), "attn_cross_fwd")
    return ctx, probs


def attn_cross_bwd(q, kv, probs, dctx, *, B, S, H, dh, drop_p=0.0, drop_site=0, rng=None, dkv=None):
    """``kv`` / ``dkv`` may be column views of wider buffers (row strides ld_kv / ld_dkv); ``dkv`` None allocates it."""
    _lib.require_gpu()
    dq = torch.empty_like(q)
    if dkv is None:
        dkv = torch.empty(kv.shape, dtype=torch.float32, device=kv.device)
    check(load().slnlp_attn_cross_bwd(ptr(q), ptr(kv), kv.stride(0), ptr(probs), ptr(dctx), B, S, H, dh, ptr(dq),
                                      ptr(dkv), dkv.stride(0), drop_p, drop_site, ptr(rng), stream_ptr()),
          "attn_cross_bwd")
    return dq, dkv


def _attn_ex_outputs(what, like_shape, device, want_planes, planes_only, want_q8, out, key):
    """The fp32 output (None under ``planes_only``), its planes and its q8 plane for the ``attn_*_ex`` wrappers; ``out`` may hold
    any of them pre-allocated (``key``, "planes" = (hi, lo), "q8"), e.g. pre-filled or padded buffers of a test."""
    out = dict(out or {})
    want_planes = want_planes or planes_only or want_q8 or "planes" in out
    fp32 = None if planes_only else out.get(key)
    if fp32 is None and not planes_only:
        fp32 = torch.empty(*like_shape, dtype=torch.float32, device=device)
    planes = out.get("planes")
    if planes is None and want_planes:
        planes = (torch.empty(*like_shape, dtype=torch.int16, device=device), torch.empty(*like_shape, dtype=torch.int16, device=device))
    q8 = out.get("q8")
    if q8 is None and want_q8:
        q8 = torch.empty(*like_shape, dtype=torch.uint8, device=device)
    for t in (fp32,) + tuple(planes or ()) + (q8,):
        assert t is None or (t.stride(-1) == 1 and t.stride(0) == like_shape[-1]), f"{what}: outputs have the fp32 tensor's row stride"
    return fp32, planes, q8


def attn_self_fwd_ex(qkv, ids, pad_idx, *, B, S, H, dh, causal=True, drop_p=0.0, drop_site=0, rng=None, want_planes=False,
                     planes_only=False, want_q8=False, out=None):
    """``attn_self_fwd`` as the plans call it (``slnlp_attn_self_fwd_ex``) -> dict of ctx (None under ``planes_only``: the call
    passes a null fp32 output), probs, planes ((hi, lo) int16 bit patterns | None) and q8 (uint8 e4m3 | None).  ``ids`` may be a
    view whose row stride is not S.  ``out``: a dict with any of ctx / probs / planes / q8 to write into."""
    _lib.require_gpu()
    E = H * dh
    ctx, planes, q8 = _attn_ex_outputs("attn_self_fwd_ex", (S * B, E), qkv.device, want_planes, planes_only, want_q8, out, "ctx")
    probs = (out or {}).get("probs")
    if probs is None:
        probs = torch.empty(B, H, S, S, dtype=torch.float32, device=qkv.device)
    hi, lo = planes or (None, None)
    check(load().slnlp_attn_self_fwd_ex(ptr(qkv), ptr(ids), ids.stride(0) if ids is not None else 0, pad_idx, int(causal), B, S, H, dh,
                                        ptr(ctx), ptr(probs), drop_p, drop_site, ptr(rng), ptr(hi), ptr(lo), ptr(q8), stream_ptr()),
          "attn_self_fwd_ex")
    return dict(ctx=ctx, probs=probs, planes=planes, q8=q8)


def attn_self_bwd_ex(qkv, probs, dctx, *, B, S, H, dh, drop_p=0.0, drop_site=0, rng=None, want_planes=False, planes_only=False,
                     out=None):
    """``attn_self_bwd`` as the plans call it (``slnlp_attn_self_bwd_ex``) -> dict of dqkv (None under ``planes_only``) and planes
    ((hi, lo) int16 | None), row stride 3E.  ``out``: a dict with dqkv / planes to write into."""
    _lib.require_gpu()
    dqkv, planes, _ = _attn_ex_outputs("attn_self_bwd_ex", (S * B, 3 * H * dh), qkv.device, want_planes, planes_only, False, out, "dqkv")
    scratch = None
    if S > 64:
        scratch = torch.empty(int(load().slnlp_attn_long_scratch_bytes(B, S, H)), dtype=torch.uint8, device=qkv.device)
    hi, lo = planes or (None, None)
    check(load().slnlp_attn_self_bwd_ex(ptr(qkv), ptr(probs), ptr(dctx), B, S, H, dh, ptr(dqkv), drop_p, drop_site, ptr(rng),
                                        ptr(scratch), ptr(hi), ptr(lo), stream_ptr()), "attn_self_bwd_ex")
    return dict(dqkv=dqkv, planes=planes)


def attn_cross_bwd_ex(q, kv, probs, dctx, *, B, S, H, dh, drop_p=0.0, drop_site=0, rng=None, want_planes=False, out=None):
    """``attn_cross_bwd`` with the planes of dkv (``slnlp_attn_cross_bwd_ex``) -> dict of dq, dkv and planes ((hi, lo) int16 | None).
    ``out``: a dict with dkv / planes to write into; the planes have dkv's row stride (column views of wider buffers are fine)."""
    _lib.require_gpu()
    out = dict(out or {})
    dq = torch.empty_like(q)
    dkv = out.get("dkv")
    if dkv is None:
        dkv = torch.empty(kv.shape, dtype=torch.float32, device=kv.device)
    planes = out.get("planes")
    if planes is None and want_planes:
        planes = (torch.empty(dkv.shape, dtype=torch.int16, device=kv.device), torch.empty(dkv.shape, dtype=torch.int16, device=kv.device))
    for t in planes or ():
        assert t.stride(0) == dkv.stride(0) and t.stride(1) == 1, "attn_cross_bwd_ex: the planes have dkv's row stride"
    hi, lo = planes or (None, None)
    check(load().slnlp_attn_cross_bwd_ex(ptr(q), ptr(kv), kv.stride(0), ptr(probs), ptr(dctx), B, S, H, dh, ptr(dq), ptr(dkv),
                                         dkv.stride(0), drop_p, drop_site, ptr(rng), ptr(hi), ptr(lo), stream_ptr()),
          "attn_cross_bwd_ex")
    return dict(dq=dq, dkv=dkv, planes=planes)


def attn_mem_fwd(qk, mem, bv, *, B, S, H, dh, drop_p=0.0, drop_site=0, rng=None, out=None):
    """Cross-attention over the unprojected memory, forward (``slnlp_attn_mem_fwd``): qk [B*H, E], mem [S*B, E], bv [E] ->
    (mbar [B*H, E], psum [B*H], probs [B*H, S], ctx0 [B, E]); ``out``: those four tensors to write into, or None."""
    _lib.require_gpu()
    E = H * dh
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=qk.device)
    mbar, psum, probs, ctx0 = out if out is not None else (new(B * H, E), new(B * H), new(B * H, S), new(B, E))
    check(load().slnlp_attn_mem_fwd(ptr(qk), ptr(mem), ptr(bv), B, S, H, dh, ptr(mbar), ptr(psum), ptr(probs), ptr(ctx0), drop_p,
                                    drop_site, ptr(rng), stream_ptr()), "attn_mem_fwd")
    return mbar, psum, probs, ctx0


def attn_mem_bwd(mem, bv, probs, psum, qk, dmbar, dctx, *, B, S, H, dh, drop_p=0.0, drop_site=0, rng=None, want_dmem=True, dmem=None,
                 accumulate=False, out=None):
    """Its backward (``slnlp_attn_mem_bwd``) -> (dsc [B*H, S], dqk [B*H, E], dcp [B, E], dbv [E], dmem [S*B, E] | None).
    ``want_dmem`` False passes a null d memory: the launch that writes it and dbv is left to ``attn_mem_dmem_all``.  ``dmem``
    None allocates it; ``accumulate`` adds onto the ``dmem`` given.  ``out``: (dsc, dqk, dcp, dbv) to write into, or None."""
    _lib.require_gpu()
    E = H * dh
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=mem.device)
    dsc, dqk, dcp, dbv = out if out is not None else (new(B * H, S), new(B * H, E), new(B, E), new(E))
    if not want_dmem:
        dmem = None
    elif dmem is None:
        assert not accumulate, "attn_mem_bwd: accumulate needs the d memory to add onto"
        dmem = new(S * B, E)
    check(load().slnlp_attn_mem_bwd(ptr(mem), ptr(bv), ptr(probs), ptr(psum), ptr(qk), ptr(dmbar), ptr(dctx), B, S, H, dh, ptr(dsc),
                                    ptr(dqk), ptr(dcp), ptr(dbv), ptr(dmem), int(bool(accumulate)), drop_p, drop_site, ptr(rng),
                                    stream_ptr()), "attn_mem_bwd")
    return dsc, dqk, dcp, dbv, dmem


def attn_mem_dmem_all(layers, *, B, S, H, dh, drop_p=0.0, rng=None, dmem=None):
    """d memory of all decoder layers and every layer's d bv in one launch (``slnlp_attn_mem_dmem_all``).  ``layers``: per layer
    a dict of the tensors probs, dsc, dmbar, qk, dcp, dbv (dbv is written) and the int drop_site.  -> (dmem [S*B, E], table): the
    device table of the layers' pointers, which the caller keeps until the launch has run."""
    _lib.require_gpu()
    n = len(layers)
    host = (_lib.XmemDmemLayer * n)(*[_lib.XmemDmemLayer(*[ptr(L[k]) for k in ("probs", "dsc", "dmbar", "qk", "dcp", "dbv")],
                                                         int(L["drop_site"]), 0) for L in layers])
    device = layers[0]["probs"].device
    table = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(device)
    if dmem is None:
        dmem = torch.empty(S * B, H * dh, dtype=torch.float32, device=device)
    check(load().slnlp_attn_mem_dmem_all(ptr(table), n, B, S, H, dh, ptr(dmem), drop_p, ptr(rng), stream_ptr()), "attn_mem_dmem_all")
    return dmem, table


def set_xmem_heads(hp):
    """Heads per workgroup of the two kernels above: 0 automatic, 1 / 2 / 4 forced (``slnlp_set_xmem_heads``)."""
    check(load().slnlp_set_xmem_heads(int(hp)), "set_xmem_heads")


def layernorm_fwd(x, gamma, beta, eps=1e-5):
    _lib.require_gpu()
    rows, E = x.shape
    y = torch.empty_like(x)
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    check(load().slnlp_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), rows, E, eps, ptr(y), ptr(stats), stream_ptr()),
          "layernorm_fwd")
    return y, stats


def layernorm_bwd(dy, x, gamma, stats, *, add_to_dx=None, want_drop=False, drop_p=0.0, drop_site=0, rng=None):
    """-> (dx, dx_drop | None, dgamma, dbeta)"""
    _lib.require_gpu()
    rows, E = x.shape
    dx = torch.empty_like(x)
    dxd = torch.empty_like(x) if want_drop else None
    partial = torch.empty(1024, 2, E, dtype=torch.float32, device=x.device)     # SLNLP_LN_MAX_PARTIALS chunks
    nblk = C.c_int32(0)
    check(load().slnlp_layernorm_bwd(ptr(dy), ptr(x), ptr(gamma), ptr(stats), rows, E, ptr(add_to_dx), ptr(dx),
                                     ptr(dxd), drop_p, drop_site, ptr(rng), ptr(partial), C.byref(nblk),
                                     stream_ptr()), "layernorm_bwd")
    dg = torch.empty(E, dtype=torch.float32, device=x.device)
    db = torch.empty(E, dtype=torch.float32, device=x.device)
    ent = _lib.LnReduceEntry(ptr(partial), ptr(dg), ptr(db), nblk.value, E)
    table = torch.frombuffer(bytearray(bytes(ent)), dtype=torch.uint8).to(x.device)
    check(load().slnlp_ln_param_reduce(ptr(table), 1, E, stream_ptr()), "ln_param_reduce")
    torch.cuda.current_stream().synchronize()  # `table` must outlive the launch
    return dx, dxd, dg, db


def layernorm_fwd_ex(x, gamma, beta, eps=1e-5, *, want_planes=False):
    """``layernorm_fwd`` with the output's bf16 planes (``slnlp_layernorm_fwd_ex``) -> (y, stats, (hi, lo) | None)"""
    _lib.require_gpu()
    rows, E = x.shape
    y = torch.empty_like(x)
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    hi, lo = planes = _plane_pair(y) if want_planes else (None, None)
    check(load().slnlp_layernorm_fwd_ex(ptr(x), ptr(gamma), ptr(beta), rows, E, eps, ptr(y), ptr(stats), ptr(hi), ptr(lo), stream_ptr()),
          "layernorm_fwd_ex")
    return y, stats, (planes if want_planes else None)


def layernorm_bwd_ex(dy, x, gamma, stats, *, add_to_dx=None, want_drop=False, drop_p=0.0, drop_site=0, rng=None, full_rows=0,
                     partial=None, want_planes=False, want_drop_planes=False):
    """``slnlp_layernorm_bwd_ex``: the row kernel alone, as the plans launch it -> dict of dx, dx_drop | None (``want_drop``),
    planes / drop_planes ((hi, lo) int16 | None) and nblk.  ``partial`` ([>= nblk, 2, E] fp32, or None: no column sums) receives the
    (dgamma, dbeta) chunk sums, whose chunks follow ``full_rows`` (0: this call's rows); ``ln_param_reduce`` adds them."""
    _lib.require_gpu()
    rows, E = x.shape
    dx = torch.empty_like(x)
    dxd = torch.empty_like(x) if want_drop else None
    planes = _plane_pair(dx) if want_planes else None
    dplanes = _plane_pair(dx) if want_drop_planes else None
    nblk = C.c_int32(0)
    check(load().slnlp_layernorm_bwd_ex(ptr(dy), ptr(x), ptr(gamma), ptr(stats), rows, E, ptr(add_to_dx), ptr(dx), ptr(dxd), drop_p,
                                        drop_site, ptr(rng), ptr(partial), C.byref(nblk), int(full_rows),
                                        *[ptr(t) for t in (planes or (None, None))], *[ptr(t) for t in (dplanes or (None, None))],
                                        stream_ptr()), "layernorm_bwd_ex")
    return dict(dx=dx, dx_drop=dxd, planes=planes, drop_planes=dplanes, nblk=nblk.value)


def _device_table(structs, device):
    """A ctypes array of table entries, uploaded; the caller keeps the tensor until the launch that reads it has run."""
    return torch.frombuffer(bytearray(bytes(structs)), dtype=torch.uint8).to(device)


def ln_param_partial(entries, *, E, rows_enc=0, rows_dec=0, full_rows_enc=0, full_rows_dec=0):
    """The (dgamma, dbeta) chunk sums of several LayerNorms in one table-driven launch (``slnlp_ln_param_partial``).
    ``entries``: per LayerNorm a dict of the tensors dy, x, stats, partial (written) and the flag dec."""
    _lib.require_gpu()
    n = len(entries)
    host = (_lib.LnPartialEntry * n)(*[_lib.LnPartialEntry(ptr(e["dy"]), ptr(e["x"]), ptr(e["stats"]), ptr(e["partial"]),
                                                           int(bool(e["dec"])), 0) for e in entries])
    table = _device_table(host, entries[0]["dy"].device)
    check(load().slnlp_ln_param_partial(ptr(table), n, E, rows_enc, rows_dec, full_rows_enc, full_rows_dec, stream_ptr()), "ln_param_partial")
    torch.cuda.current_stream().synchronize()  # `table` must outlive the launch


def ln_param_reduce(entries, max_E):
    """(dgamma, dbeta) of several LayerNorms from their chunk sums in one launch (``slnlp_ln_param_reduce``).  ``entries``: per
    LayerNorm a dict of the tensors partial [nblk, 2, E], dgamma, dbeta (written) and the ints nblk, E."""
    _lib.require_gpu()
    n = len(entries)
    host = (_lib.LnReduceEntry * n)(*[_lib.LnReduceEntry(ptr(e["partial"]), ptr(e["dgamma"]), ptr(e["dbeta"]), int(e["nblk"]), int(e["E"]))
                                      for e in entries])
    table = _device_table(host, entries[0]["partial"].device)
    check(load().slnlp_ln_param_reduce(ptr(table), n, max_E, stream_ptr()), "ln_param_reduce")
    torch.cuda.current_stream().synchronize()  # `table` must outlive the launch


def _dlogits(dlogits, want_grad, B, V, device):
    """The gradient output of the criterion: a [B, >= V] fp32 view to write into (its row stride is ld_dlogits), a new [B, V], or None."""
    if dlogits is not None:
        assert dlogits.shape == (B, V) and dlogits.stride(1) == 1, "dlogits: a [B, V] view with unit column stride"
        return dlogits
    return torch.empty(B, V, dtype=torch.float32, device=device) if want_grad else None


def lsm_nll(logits, y, ignore_index, *, want_grad=True, dlogits=None):
    """-> (logp [B,V], loss [1], dlogits [B,V] | None)"""
    _lib.require_gpu()
    B, V = logits.shape
    logp = torch.empty(B, V, dtype=torch.float32, device=logits.device)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dl = _dlogits(dlogits, want_grad, B, V, logits.device)
    rows = torch.empty(B, dtype=torch.float32, device=logits.device)
    check(load().slnlp_lsm_nll(ptr(logits), logits.stride(0), ptr(y), B, V, ignore_index, ptr(logp), ptr(loss),
                               ptr(dl), V if dl is None else dl.stride(0), ptr(rows), stream_ptr()), "lsm_nll")
    return logp, loss, dl


def lsm_nll_ex(logits, y, ignore_index, *, weight=None, label_smoothing=0.0, reduction="mean", want_grad=True, dlogits=None):
    """``lsm_nll`` with CrossEntropyLoss's ``weight`` ([V] fp32 on the device, or None), ``label_smoothing`` and
    ``reduction`` ("mean" / "sum") -> (logp [B,V], loss [1], dlogits [B,V] | None)"""
    _lib.require_gpu()
    B, V = logits.shape
    logp = torch.empty(B, V, dtype=torch.float32, device=logits.device)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dl = _dlogits(dlogits, want_grad, B, V, logits.device)
    rows = torch.empty(B, dtype=torch.float32, device=logits.device)
    w = None if weight is None else weight.to(logits.device, torch.float32).contiguous()
    check(load().slnlp_lsm_nll_ex(ptr(logits), logits.stride(0), ptr(y), B, V, ignore_index, ptr(w), float(label_smoothing),
                                  _lib.REDUCTIONS[reduction], ptr(logp), ptr(loss), ptr(dl), V if dl is None else dl.stride(0), ptr(rows),
                                  stream_ptr()), "lsm_nll_ex")
    return logp, loss, dl


def lsm_bwd(logp, dlogp, *, dlogits=None):
    _lib.require_gpu()
    B, V = logp.shape
    out = _dlogits(dlogits, True, B, V, logp.device)
    check(load().slnlp_lsm_bwd(ptr(logp), ptr(dlogp), B, V, ptr(out), out.stride(0), stream_ptr()), "lsm_bwd")
    return out


def clip_sgd_step(params, grads, buf, lr_dev, *, momentum=0.9, max_norm=0.5, rng=None):
    """In-place update of flat fp32 arenas; returns the pre-clip norm tensor [1]."""
    _lib.require_gpu()
    partials = torch.empty(1024, dtype=torch.float32, device=params.device)
    norm = torch.empty(1, dtype=torch.float32, device=params.device)
    check(load().slnlp_clip_sgd_step(ptr(params), ptr(grads), ptr(buf), params.numel(), ptr(lr_dev), momentum,
                                     max_norm, ptr(partials), ptr(norm), ptr(rng), stream_ptr()), "clip_sgd_step")
    return norm


def clip_adam_step(params, grads, exp_avg, exp_avg_sq, lr_dev, step_count, *, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.5):
    """In-place clip + Adam on flat fp32 arenas; ``step_count`` [1] float (device) is advanced.  Returns the pre-clip norm [1]."""
    _lib.require_gpu()
    partials = torch.empty(1024, dtype=torch.float32, device=params.device)
    norm = torch.empty(1, dtype=torch.float32, device=params.device)
    check(load().slnlp_clip_adam_step(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), ptr(lr_dev), betas[0], betas[1],
                                      eps, weight_decay, max_norm, ptr(partials), ptr(norm), ptr(step_count), stream_ptr()), "clip_adam_step")
    return norm


def clip_sgd_step_ex(params, grads, buf, lr_dev, step_count, *, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False,
                     max_norm=0.5, skip=(0, 0)):
    """clip + torch.optim.SGD with dampening / weight decay / Nesterov; ``step_count`` [1] float (device) counts the steps
    (0 before the first) and is advanced; floats [skip[0], skip[1]) stay untouched.  Returns the pre-clip norm [1]."""
    _lib.require_gpu()
    partials = torch.empty(1024, dtype=torch.float32, device=params.device)
    norm = torch.empty(1, dtype=torch.float32, device=params.device)
    check(load().slnlp_clip_sgd_step_ex(ptr(params), ptr(grads), ptr(buf), params.numel(), ptr(lr_dev), momentum, dampening,
                                        weight_decay, int(bool(nesterov)), max_norm, ptr(partials), ptr(norm), ptr(step_count),
                                        skip[0], skip[1], stream_ptr()), "clip_sgd_step_ex")
    return norm


def clip_adamw_step(params, grads, exp_avg, exp_avg_sq, lr_dev, step_count, *, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                    max_norm=0.5, skip=(0, 0)):
    """clip + torch.optim.AdamW on flat fp32 arenas (floats [skip[0], skip[1]) untouched).  Returns the pre-clip norm [1]."""
    _lib.require_gpu()
    partials = torch.empty(1024, dtype=torch.float32, device=params.device)
    norm = torch.empty(1, dtype=torch.float32, device=params.device)
    check(load().slnlp_clip_adamw_step(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), ptr(lr_dev), betas[0],
                                       betas[1], eps, weight_decay, max_norm, ptr(partials), ptr(norm), ptr(step_count), skip[0], skip[1],
                                       stream_ptr()), "clip_adamw_step")
    return norm


def average_step(avg, params, count, *, kind="swa", decay=0.0, skip=(0, 0)):
    """Feed ``params`` into the running average ``avg`` (flat fp32 arenas, in place): a bit copy while ``count`` [1] float
    (device) is 0, then ``kind`` "swa" (``AveragedModel``'s default ``avg_fn``) or "ema" (``get_ema_multi_avg_fn(decay)``);
    floats ``skip`` [begin, end) are copied.  ``count`` is advanced on the device; no host wait."""
    _lib.require_gpu()
    check(load().slnlp_average_step(ptr(avg), ptr(params), params.numel(), ptr(count), _lib.AVERAGE_KINDS[kind], float(decay),
                                    int(skip[0]), int(skip[1]), stream_ptr()), "average_step")


def swap_arenas(a, b):
    """Exchange two flat fp32 arenas in place (one launch); two swaps restore every bit."""
    _lib.require_gpu()
    check(load().slnlp_swap_arenas(ptr(a), ptr(b), a.numel(), stream_ptr()), "swap_arenas")


def score_buffers(N, V, device):
    """The four output tensors of ``score_rows`` for an [N, V] epoch: slices of ONE allocation, so ``score_download`` is one copy."""
    return _packed.Packed(torch.int32, _score_pieces(N, V), device).views()


def _score_pieces(N, V):
    return (("pred", torch.int32, N, 4), ("picked", torch.float32, N, 4), ("rank", torch.int32, N, 4), ("counts", torch.int32, 3 * V + 1, 4))


def score_download(out):
    """``score_rows``' four tensors as numpy arrays: one device-to-host copy when they are ``score_buffers``' slices of one
    allocation, four otherwise."""
    return _packed.download(out, torch.int32)


def score_rows(logp, y, out=None):
    """An epoch's log-probs ``logp`` float32 [N, V] (rows may be padded: ``stride(0) >= V``) and labels ``y`` int64 [N] reduced to
    ``(pred int32 [N], picked float32 [N], rank int32 [N], counts int32 [3 V + 1])``, device tensors (``slnlp_score_rows``,
    include/slnlp.h); ``out``: such a 4-tuple to fill.  Runs on the current stream of ``logp``'s device; no host wait."""
    _lib.require_gpu()
    N, V, ld = _logp_matrix("score_rows", logp)
    _labels("score_rows", y, logp.device, N)
    with torch.cuda.device(logp.device):
        if out is None:
            out = score_buffers(N, V, logp.device)
        pred, picked, rank, counts = out
        for t, dt, n in ((pred, torch.int32, N), (picked, torch.float32, N), (rank, torch.int32, N), (counts, torch.int32, 3 * V + 1)):
            _tensor("score_rows", "out", t, logp.device, dt, n,
                    f"(int32 [{N}], float32 [{N}], int32 [{N}], int32 [{3 * V + 1}]) on {logp.device}")
        check(load().slnlp_score_rows(ptr(logp), ld, ptr(y), N, V, ptr(pred), ptr(picked), ptr(rank), ptr(counts), stream_ptr()),
              "score_rows")
    return out


CAL_STATE_DOUBLES = 16                       # SLNLP_CAL_STATE_BYTES / 8: eight doubles, then eight int64


def _logp_matrix(what, logp):
    if not (logp.is_cuda and logp.dtype == torch.float32 and logp.dim() == 2 and (logp.stride(1) == 1 or logp.shape[1] == 1)):
        raise ValueError(f"{what}: logp must be a float32 [N, V] device tensor with unit column stride, got {logp.dtype} "
                         f"{tuple(logp.shape)} strides {logp.stride()} on {logp.device}")
    N, V = int(logp.shape[0]), int(logp.shape[1])
    return N, V, (int(logp.stride(0)) if N > 1 else max(V, int(logp.stride(0))))


def _tensor(what, name, t, device, dtype, shape, must_be=None):
    """The tensor contract of the judging wrappers: ``t`` on ``device``, of ``dtype``, contiguous, of ``shape`` -- a tuple, an int
    n for (n,), None for one dimension of any length.  ``must_be``: the message's wording of it where that is not the default."""
    dims = shape if isinstance(shape, tuple) else (shape,)
    if not (t.device == device and t.dtype == dtype and t.is_contiguous() and (t.dim() == 1 if shape is None else tuple(t.shape) == dims)):
        text = must_be or f"a contiguous {str(dtype)[6:]} [{', '.join(map(str, dims))}] tensor on {device}"
        raise ValueError(f"{what}: {name} must be {text}")


def _labels(what, y, device, N, or_none=""):
    _tensor(what, "y", y, device, torch.int64, N, f"a contiguous int64 [{N}] tensor on {device}{or_none}")


def _cal_state(what, state, device):
    _tensor(what, "state", state, device, torch.float64, CAL_STATE_DOUBLES)


def _scratch(what, scratch, device, doubles=None):
    """A fit's scratch: float64, one dimension (the library checks its length; ``doubles``: what the message says it takes)"""
    _tensor(what, "scratch", scratch, device, torch.float64, None,
            f"a contiguous float64 {'' if doubles is None else f'[>= {doubles}] '}tensor on {device}")


def _out_like(what, logp, out):
    """-> (out, its row stride): ``out`` -- None: a new tensor; ``logp`` itself: in place -- as a float32 matrix of ``logp``'s shape
    on its device"""
    N, V = int(logp.shape[0]), int(logp.shape[1])
    if out is None:
        out = torch.empty(N, V, dtype=torch.float32, device=logp.device)
    if out.device != logp.device or tuple(out.shape) != (N, V):
        raise ValueError(f"{what}: out must be a float32 [{N}, {V}] tensor on {logp.device}")
    return out, _logp_matrix(f"{what} (out)", out)[2]


def fit_temperature(logp, y, state=None, scratch=None):
    """Fit the temperature of ``logp`` float32 [N, V] (rows may be padded: ``stride(0) >= V``) against the labels ``y`` int64 [N]
    (``slnlp_fit_temperature``, include/slnlp.h).  Returns the device state, float64 [16] (``temperature_download`` reads it;
    its first double is beta = 1 / T, what ``scale_logp`` takes); ``state`` / ``scratch`` (float64 [>= 4 N]): buffers to use.
    Runs on the current stream of ``logp``'s device; no host wait."""
    _lib.require_gpu()
    N, V, ld = _logp_matrix("fit_temperature", logp)
    _labels("fit_temperature", y, logp.device, N)
    with torch.cuda.device(logp.device):
        if state is None:
            state = torch.empty(CAL_STATE_DOUBLES, dtype=torch.float64, device=logp.device)
        _cal_state("fit_temperature", state, logp.device)
        if scratch is None:
            scratch = torch.empty(4 * N, dtype=torch.float64, device=logp.device)
        _scratch("fit_temperature", scratch, logp.device, 4 * N)
        check(load().slnlp_fit_temperature(ptr(logp), ld, ptr(y), N, V, ptr(state), ptr(scratch), scratch.numel() * 8, stream_ptr()),
              "fit_temperature")
    return state


def temperature_state(beta, device):
    """A device state that holds only beta (and T): what ``scale_logp`` needs of a calibration read back from a checkpoint."""
    state = torch.zeros(CAL_STATE_DOUBLES, dtype=torch.float64)
    state[0], state[1] = float(beta), 1.0 / float(beta)
    return state.to(device)


def temperature_download(state):
    """``fit_temperature``'s state as a dict: {temperature, beta, nll_before, nll_after, reason ("flat" | "bound" | "gradient" |
    "step" | "cap"), iterations, rows, bad_labels}.  One device-to-host copy (it waits for the fit's launches)."""
    return _calibration_download(state, _lib.CALIBRATION_REASONS)


def _calibration_download(state, reasons):
    h = state.cpu().numpy()
    q = h.view("int64")[8:]
    return {"temperature": float(h[1]), "beta": float(h[0]), "nll_before": float(h[2]), "nll_after": float(h[3]),
            "reason": reasons[int(q[0])], "iterations": int(q[1]), "rows": int(q[2]), "bad_labels": int(q[3])}


def _positive(what, name, v, zero_ok=False):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not (0.0 <= float(v) if zero_ok else 0.0 < float(v)) or not float(v) < float("inf"):
        raise ValueError(f"{what}: {name}={v!r}, expected a finite number {'>= 0' if zero_ok else '> 0'}")
    return float(v)


def fit_bias_temperature(logp, y, bias_sd=2.0, tol=1e-10, state=None, bias=None, scratch=None):
    """Fit a temperature AND a per-class bias on ``logp`` float32 [N, V] (rows may be padded: ``stride(0) >= V``; V <= 512) against
    the labels ``y`` int64 [N] -- bias-corrected temperature scaling, the MAP estimate under a N(0, ``bias_sd``^2) prior on every
    bias (``slnlp_fit_bias_temperature``, include/slnlp.h states the damped Newton iteration).  ``tol``: the absolute bound on
    max |gradient| the search stops at.  Returns ``(state, bias)``: the device state float64 [16], laid out as
    ``fit_temperature``'s (its first double is beta), and the bias float64 [V] -- what ``shift_logp(logp, bias, state)`` takes.
    ``state`` / ``bias`` / ``scratch`` (float64, ``slnlp_fit_bias_temperature_scratch_bytes`` / 8 doubles): buffers to use.  Runs
    on the current stream of ``logp``'s device; no host wait."""
    _lib.require_gpu()
    N, V, ld = _logp_matrix("fit_bias_temperature", logp)
    _labels("fit_bias_temperature", y, logp.device, N)
    bias_sd, tol = _positive("fit_bias_temperature", "bias_sd", bias_sd), _positive("fit_bias_temperature", "tol", tol, zero_ok=True)
    with torch.cuda.device(logp.device):
        if state is None:
            state = torch.empty(CAL_STATE_DOUBLES, dtype=torch.float64, device=logp.device)
        _cal_state("fit_bias_temperature", state, logp.device)
        if bias is None:
            bias = torch.empty(V, dtype=torch.float64, device=logp.device)
        _prior_vector("fit_bias_temperature", "bias", bias, logp.device, V)
        if scratch is None:
            need = load().slnlp_fit_bias_temperature_scratch_bytes(N, V)
            check(0 if need >= 0 else 1, "fit_bias_temperature_scratch_bytes")
            scratch = torch.empty(need // 8, dtype=torch.float64, device=logp.device)
        _scratch("fit_bias_temperature", scratch, logp.device)
        check(load().slnlp_fit_bias_temperature(ptr(logp), ld, ptr(y), N, V, bias_sd, tol, ptr(state), ptr(bias), ptr(scratch),
                                                scratch.numel() * 8, stream_ptr()), "fit_bias_temperature")
    return state, bias


def bias_temperature_state(beta, bias, device):
    """``(state, bias)`` on ``device`` holding only beta (and T) and the bias: what ``shift_logp`` needs of a bias calibration read
    back from a checkpoint."""
    import numpy as np
    return temperature_state(beta, device), torch.from_numpy(np.ascontiguousarray(np.asarray(bias, dtype=np.float64))).to(device)


def bias_temperature_download(state, bias, bias_sd):
    """``fit_bias_temperature``'s result as a dict: ``temperature_download``'s -- ``iterations`` counts the evaluations, rejected
    candidates included; ``nll_before`` / ``nll_after`` are the mean log-loss at (1, 0) and at the result, WITHOUT the penalty --
    plus ``method`` "bias_temperature", ``bias_sd``, ``bias`` (float64 [V]) and ``penalty``, (1 / (2 bias_sd^2 rows)) sum bias^2.
    Two device-to-host copies (the first waits for the fit's launches)."""
    info = _calibration_download(state, _lib.BIAS_CALIBRATION_REASONS)
    b = bias.cpu().numpy().copy()
    info.update(method="bias_temperature", bias_sd=float(bias_sd), bias=b,
                penalty=0.5 / (float(bias_sd) ** 2 * info["rows"]) * float((b * b).sum()) if info["rows"] else 0.0)
    return info


def scale_logp(logp, state, out=None):
    """The calibrated log-probs ``beta logp - logsumexp(beta logp)`` per row, beta read on the device from ``state``'s first double
    (``slnlp_scale_logp``).  ``out``: a float32 [N, V] tensor to fill -- ``logp`` itself for in place; default a new one.  Runs on
    the current stream of ``logp``'s device; no host wait."""
    _lib.require_gpu()
    N, V, ld = _logp_matrix("scale_logp", logp)
    _cal_state("scale_logp", state, logp.device)
    with torch.cuda.device(logp.device):
        out, ld_out = _out_like("scale_logp", logp, out)
        check(load().slnlp_scale_logp(ptr(logp), ld, N, V, ptr(state), ptr(out), ld_out, stream_ptr()), "scale_logp")
    return out


PRIOR_STATE_DOUBLES = 16                     # SLNLP_PRIOR_STATE_BYTES / 8: eight doubles, then eight int64


def _prior_vector(what, name, t, device, V):
    _tensor(what, name, t, device, torch.float64, V)


def fit_priors(logp, log_source, state=None, max_iter=200, tol=1e-6, out=None, scratch=None):
    """Re-estimate the class priors of the UNLABELLED rows ``logp`` float32 [N, V] (rows may be padded: ``stride(0) >= V``) by EM
    (``slnlp_fit_priors``, include/slnlp.h).  ``log_source``: float64 [V] on the device, ln of the priors the log-probs were
    trained under (finite).  ``state``: a calibration state whose beta is read on the device, so the EM runs on softmax(beta
    logp); None: beta = 1.  ``max_iter`` in 0..1024 (0: one evaluation, the priors are the mean prediction), ``tol`` finite and
    >= 0.  Returns ONE float64 [3 V + 16] device tensor (``priors_download`` reads it): the table -- the mean prediction, the
    priors, the log-ratio ln(priors / source) that ``shift_logp`` takes, ``out[2 * V:3 * V]`` -- then the 16 words of the fit's
    state.  ``out`` / ``scratch`` (float64 [>= 2 N + V]): buffers to use.  Runs on the current stream of ``logp``'s device; no
    host wait."""
    _lib.require_gpu()
    N, V, ld = _logp_matrix("fit_priors", logp)
    _prior_vector("fit_priors", "log_source", log_source, logp.device, V)
    max_iter = _int_in("fit_priors", "max_iter", max_iter, 0, _lib.PRIOR_MAX_ITER)
    tol = _positive("fit_priors", "tol", tol, zero_ok=True)
    if state is not None:
        _cal_state("fit_priors", state, logp.device)
    with torch.cuda.device(logp.device):
        if out is None:
            out = torch.empty(3 * V + PRIOR_STATE_DOUBLES, dtype=torch.float64, device=logp.device)
        _prior_vector("fit_priors", "out", out, logp.device, 3 * V + PRIOR_STATE_DOUBLES)
        if scratch is None:
            scratch = torch.empty(2 * N + V, dtype=torch.float64, device=logp.device)
        _scratch("fit_priors", scratch, logp.device, 2 * N + V)
        check(load().slnlp_fit_priors(ptr(logp), ld, N, V, ptr(state), ptr(log_source), max_iter, tol, ptr(out), ptr(out[3 * V:]),
                                      ptr(scratch), scratch.numel() * 8, stream_ptr()), "fit_priors")
    return out


def priors_download(out):
    """``fit_priors``' result as a dict: {priors, mean_proba, log_ratio (float64 [V] each), gain, d, reason ("tol" | "cap" |
    "empty"), iterations, rows, nan_rows}.  ONE device-to-host copy (it waits for the fit's launches)."""
    h = out.cpu().numpy()
    V = (h.size - PRIOR_STATE_DOUBLES) // 3
    s = h[3 * V:]
    q = s.view("int64")[8:]
    return {"priors": h[V:2 * V].copy(), "mean_proba": h[:V].copy(), "log_ratio": h[2 * V:3 * V].copy(), "gain": float(s[0]),
            "d": float(s[1]), "reason": _lib.PRIOR_REASONS[int(q[0])], "iterations": int(q[1]), "rows": int(q[2]), "nan_rows": int(q[3])}


def shift_logp(logp, log_w, state=None, out=None):
    """The log-probs under other class priors, ``(beta logp + log_w) - logsumexp(beta logp + log_w)`` per row (``slnlp_shift_logp``):
    ``log_w`` float64 [V] on the device, ln(target prior / source prior) -- ``fit_priors``' ``out[2 * V:3 * V]``; ``state``: a
    calibration state whose beta is read on the device (None: beta = 1).  ``out``: a float32 [N, V] tensor to fill -- ``logp``
    itself for in place; default a new one.  Runs on the current stream of ``logp``'s device; no host wait."""
    _lib.require_gpu()
    N, V, ld = _logp_matrix("shift_logp", logp)
    _prior_vector("shift_logp", "log_w", log_w, logp.device, V)
    if state is not None:
        _cal_state("shift_logp", state, logp.device)
    with torch.cuda.device(logp.device):
        out, ld_out = _out_like("shift_logp", logp, out)
        check(load().slnlp_shift_logp(ptr(logp), ld, N, V, ptr(state), ptr(log_w), ptr(out), ld_out, stream_ptr()), "shift_logp")
    return out


def reliability_buffers(N, bins, device):
    """The two output tensors of ``reliability_rows`` for N rows and ``bins`` bins -- rows float64 [N, 4], table float64
    [bins + 1, 4] -- as slices of ONE allocation, so ``reliability_download`` is one copy."""
    return _packed.Packed(torch.float64, (("rows", torch.float64, (N, 4), 8), ("table", torch.float64, (bins + 1, 4), 8)), device).views()


def reliability_rows(logp, y, bins=15, state=None, out=None):
    """The reliability terms of ``logp`` float32 [N, V] (rows may be padded: ``stride(0) >= V``) against the labels ``y`` int64 [N]
    (``slnlp_reliability_rows``, include/slnlp.h): ``(rows float64 [N, 4], table float64 [bins + 1, 4])``, device tensors that are
    slices of one allocation.  ``state``: a calibration state (``fit_temperature`` / ``temperature_state``) whose beta is read on
    the device, so the terms are those of softmax(beta logp); None: beta = 1.  ``out``: such a pair to fill.  Runs on the current
    stream of ``logp``'s device; no host wait."""
    _lib.require_gpu()
    N, V, ld = _logp_matrix("reliability_rows", logp)
    _labels("reliability_rows", y, logp.device, N)
    if isinstance(bins, bool) or not isinstance(bins, numbers.Integral) or not 1 <= bins <= _lib.REL_MAX_BINS:
        raise ValueError(f"reliability_rows: bins={bins!r}, expected an integer in 1..{_lib.REL_MAX_BINS}")
    bins = int(bins)
    if state is not None:
        _cal_state("reliability_rows", state, logp.device)
    with torch.cuda.device(logp.device):
        if out is None:
            out = reliability_buffers(N, bins, logp.device)
        rows, table = out
        for t, shape in ((rows, (N, 4)), (table, (bins + 1, 4))):
            _tensor("reliability_rows", "out", t, logp.device, torch.float64, shape, f"(float64 [{N}, 4], float64 [{bins + 1}, 4]) on {logp.device}")
        check(load().slnlp_reliability_rows(ptr(logp), ld, ptr(y), N, V, bins, ptr(state), ptr(rows), ptr(table), stream_ptr()),
              "reliability_rows")
    return out


def reliability_download(out):
    """``reliability_rows``' result as a dict (``metrics.reliability_from_table`` forms it on the host, in fp64, from the table):
    {ece, mce, brier, nll, accuracy, confidence, rows, bad_labels, nan_rows, bins: {count, confidence, accuracy}}.  ONE
    device-to-host copy, of the table (it waits for the two launches); the per-row terms stay on the device."""
    from . import metrics
    return metrics.reliability_from_table(out[1].cpu().numpy())


def ranking_buffers(N, V, device, per_row=True):
    """The two output tensors of ``ranking_rows`` for an [N, V] set of log-probs -- rows int32 [N, 4] (None with
    ``per_row=False``), table float64 [V + 1, 4] -- as slices of ONE allocation: the table comes first, so it is 32-byte aligned
    and ``ranking_download`` copies it alone."""
    p = _packed.Packed(torch.float64, (("table", torch.float64, (V + 1, 4), 8),) + ((("rows", torch.int32, (N, 4), 8),) if per_row else ()), device)
    return (p.view("rows") if per_row else None), p.view("table")


def ranking_rows(logp, y, out=None, per_row=True):
    """What the one-vs-rest ROC AUC and average precision of every class are functions of, from ``logp`` float32 [N, V] (rows may
    be padded: ``stride(0) >= V``) and the labels ``y`` int64 [N] (``slnlp_ranking_rows``, include/slnlp.h): ``(rows int32 [N, 4],
    table float64 [V + 1, 4])``, device tensors; rows = (negatives above, negatives tied, positives at or above, code) per
    sample, None with ``per_row=False`` (the kernel then writes the table alone).  ``out``: such a pair to fill (its rows may be
    None, whatever ``per_row`` says).  Runs on the current stream of ``logp``'s device; no host wait."""
    _lib.require_gpu()
    N, V, ld = _logp_matrix("ranking_rows", logp)
    _labels("ranking_rows", y, logp.device, N)
    if N > _lib.RANK_MAX_ROWS:
        raise ValueError(f"ranking_rows: {N} rows, the pair counts are exact for at most {_lib.RANK_MAX_ROWS}")
    with torch.cuda.device(logp.device):
        if out is None:
            out = ranking_buffers(N, V, logp.device, per_row=bool(per_row))
        rows, table = out
        must_be = f"(int32 [{N}, 4] or None, float64 [{V + 1}, 4]) on {logp.device}"
        _tensor("ranking_rows", "out", table, logp.device, torch.float64, (V + 1, 4), must_be)
        if rows is not None:
            _tensor("ranking_rows", "out", rows, logp.device, torch.int32, (N, 4), must_be)
        check(load().slnlp_ranking_rows(ptr(logp), ld, ptr(y), N, V, ptr(rows), ptr(table), stream_ptr()), "ranking_rows")
    return out


def ranking_download(out, per_row=False):
    """``ranking_rows``' result as a dict (``metrics.ranking_from_table`` forms it on the host, in fp64, from the table):
    {auc_macro, auc_weighted, ap_macro, ap_weighted, classes_scored, auc [V], ap [V], support [V], rows, bad_labels, nan_classes}.
    ONE device-to-host copy, of the table (it waits for the launch); ``per_row=True`` adds ``per_row``, the int32 [N, 4] rows (a
    second copy)."""
    from . import metrics
    res = metrics.ranking_from_table(out[1].cpu().numpy())
    if per_row:
        if out[0] is None:
            raise ValueError("ranking_download: per_row=True, but the call formed no rows (ranking_rows(per_row=False))")
        res["per_row"] = out[0].cpu().numpy()
    return res


def _int_in(what, name, value, lo, hi):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or not lo <= value <= hi:
        raise ValueError(f"{what}: {name}={value!r}, expected an integer in {lo}..{hi}")
    return int(value)


def conformal_buffers(N, V, device, sets=True):
    """Every device buffer of one conformal pass over an [N, V] set of log-probs, as slices of ONE int64 allocation:

        state float64 [4] | table int64 [V + 1, 4] | score float64 [N] | rows int32 [N, 4] | sets int32 [N, ceil(V / 32)]

    (one pad entry in front of rows where that keeps them 16-byte aligned; ``sets`` None with ``sets=False``).  The state and
    the table come first, so ``conformal_download`` copies them alone; the set words are uint32 bit masks held in int32."""
    what = "conformal_buffers"
    N, V = _int_in(what, "N", N, 1, 2 ** 31 - 1), _int_in(what, "V", V, 1, _lib.CONFORMAL_MAX_V)
    pieces = [("state", torch.float64, 4, 8), ("table", torch.int64, (V + 1, 4), 8), ("score", torch.float64, N, 8),
              ("rows", torch.int32, (N, 4), 16)] + ([("sets", torch.int32, (N, (V + 31) // 32), 4)] if sets else [])
    return _packed_dict(_packed.Packed(torch.int64, pieces, device), (N, V), sets=None)


def _packed_dict(p, shape, shaped=True, **more):
    """What a dict-returning ``*_buffers`` hands out: the allocation, the shape it was made for, ``packed`` (the table that laid it
    out and cuts its downloads), the keys ``more`` and every piece as a device view"""
    return {"flat": p.flat, "shape": shape, "packed": p, **more, **dict(zip(p.at, p.views(shaped=shaped)))}


def _even_ints(name, *shape):
    """An int32 piece of a buffer whose pieces are all 8-byte aligned: padded to an even length"""
    n = math.prod(shape)
    return name, torch.int32, shape, 8, n + (n & 1)


def _packed_buf(what, buf, maker, shape, device, more=0):
    """``buf`` is ``maker``'s dict for a shape that begins with ``shape`` (``more`` further entries), on ``device`` (None: any)"""
    if not (isinstance(buf, dict) and len(buf.get("shape", ())) == len(shape) + more and buf["shape"][:len(shape)] == shape
            and (device is None or buf["flat"].device == device)):
        raise ValueError(f"{what}: buf must be {maker}")


def _conformal_state(what, name, t, device):
    _tensor(what, name, t, device, torch.float64, 4)


def conformal_rows(logp, y=None, buf=None, *, method="aps", lam=0.0, k_reg=0, randomized=True, seed=0, draw=0, state=None, qhat=None):
    """The conformal scores and prediction sets of ``logp`` float32 [N, V] (rows may be padded: ``stride(0) >= V``; V <= 1024)
    (``slnlp_conformal_rows``, include/slnlp.h), into ``buf`` (``conformal_buffers``; default a new one, which is returned).
    ``y`` int64 [N] or None: with labels ``buf["score"]`` holds s(y_i) and ``buf["rows"]`` the label's rank and whether the set
    covers it.  ``method`` "lac" | "aps"; ``lam`` / ``k_reg``: the RAPS penalty; ``randomized`` / ``seed`` / ``draw``: one u per
    row from the counter-based generator.  ``state``: a calibration state whose beta is read on the device (None: beta = 1).
    ``qhat``: a float64 [4] device tensor whose first entry is the threshold (``conformal_quantile``'s state), read on the
    device; None: scores and ranks only, ``buf["sets"]`` is not written.  Runs on the current stream of ``logp``'s device; no
    host wait."""
    _lib.require_gpu()
    what = "conformal_rows"
    N, V, ld = _logp_matrix(what, logp)
    if V > _lib.CONFORMAL_MAX_V:
        raise ValueError(f"{what}: {V} classes, a row is sorted for at most {_lib.CONFORMAL_MAX_V}")
    if y is not None:
        _labels(what, y, logp.device, N, " or None")
    if method not in _lib.CONFORMAL_METHODS:
        raise ValueError(f"{what}: method={method!r}, expected one of {tuple(_lib.CONFORMAL_METHODS)}")
    seed, draw = _int_in(what, "seed", seed, 0, 2 ** 64 - 1), _int_in(what, "draw", draw, 0, 2 ** 32 - 1)
    k_reg = _int_in(what, "k_reg", k_reg, 0, 2 ** 31 - 1)
    if state is not None:
        _cal_state(what, state, logp.device)
    if qhat is not None:
        _conformal_state(what, "qhat", qhat, logp.device)
    with torch.cuda.device(logp.device):
        if buf is None:
            buf = conformal_buffers(N, V, logp.device, sets=qhat is not None)
        _packed_buf(what, buf, f"conformal_buffers({N}, {V}, {logp.device!r})", (N, V), logp.device)
        sets = buf["sets"] if qhat is not None else None
        check(load().slnlp_conformal_rows(ptr(logp), ld, ptr(y), N, V, ptr(state), _lib.CONFORMAL_METHODS[method], float(lam), k_reg,
                                          1 if randomized else 0, seed, draw, ptr(qhat), ptr(buf["score"]) if y is not None else None,
                                          ptr(buf["rows"]), ptr(sets), stream_ptr()), what)
    return buf


def conformal_quantile(buf, alpha, state=None):
    """The threshold of ``buf``'s scores (``conformal_rows`` with labels): ``state`` float64 [4] = (qhat, n, k, rows left out) --
    qhat the ceil((n + 1)(1 - alpha))-th smallest score of the n rows with code 0, +inf when there are too few
    (``slnlp_conformal_quantile``).  ``state``: the tensor to fill, default ``buf["state"]``; returned.  No host wait."""
    _lib.require_gpu()
    N, _ = buf["shape"]
    state = buf["state"] if state is None else state
    _conformal_state("conformal_quantile", "state", state, buf["flat"].device)
    with torch.cuda.device(state.device):
        check(load().slnlp_conformal_quantile(ptr(buf["score"]), ptr(buf["rows"]), N, float(alpha), ptr(state), stream_ptr()),
              "conformal_quantile")
    return state


def conformal_summary(buf, y):
    """The coverage / set-size table of ``buf``'s rows against the labels ``y`` int64 [N] (``slnlp_conformal_summary``): fills and
    returns ``buf["table"]``, int64 [V + 1, 4].  No host wait."""
    _lib.require_gpu()
    N, V = buf["shape"]
    dev = buf["flat"].device
    _labels("conformal_summary", y, dev, N)
    with torch.cuda.device(dev):
        check(load().slnlp_conformal_summary(ptr(buf["rows"]), ptr(y), N, V, ptr(buf["table"]), stream_ptr()), "conformal_summary")
    return buf["table"]


def conformal_download(buf, rows=False, sets=False, score=False):
    """What a conformal pass hands to the host: ONE device-to-host copy of the state and the table -- {qhat, n, k, excluded,
    state float64 [4], table int64 [V + 1, 4]} (a piece no call has written yet holds whatever the allocation held) -- and, only
    on request, one further copy each for ``rows`` int32 [N, 4], ``sets`` uint32 [N, W] and ``score`` float64 [N]."""
    import numpy as np
    out = buf["packed"].cut("state", "table")
    st = out["state"]
    out.update(qhat=float(st[0]), n=st[1], k=st[2], excluded=st[3])
    if rows:
        out["rows"] = buf["rows"].cpu().numpy()
    if sets:
        if buf["sets"] is None:
            raise ValueError("conformal_download: sets=True, but the buffers hold none (conformal_buffers(sets=False))")
        out["sets"] = buf["sets"].cpu().numpy().view(np.uint32)
    if score:
        out["score"] = buf["score"].cpu().numpy()
    return out


def selective_buffers(N, device):
    """Every device buffer of one selective-prediction pass over N rows, as slices of ONE float64 allocation:

        table float64 [40 + ceil(N / 2048)] | kappa float64 [N] | rows int32 [N, 4] | counts int32 [N, 2]

    (one pad entry in front of rows where that keeps them 16-byte aligned): 32 bytes a row, which ``selective_download`` brings
    over in one copy."""
    N = _int_in("selective_buffers", "N", N, 1, _lib.SEL_MAX_ROWS)
    head = _lib.SEL_TABLE_HEAD + (N + _lib.SEL_CHUNK - 1) // _lib.SEL_CHUNK
    p = _packed.Packed(torch.float64, (("table", torch.float64, head, 8), ("kappa", torch.float64, N, 8), ("rows", torch.int32, (N, 4), 16),
                                       ("counts", torch.int32, (N, 2), 4)), device)
    return _packed_dict(p, (N,), at=(p.begin("kappa"), p.begin("rows"), p.begin("counts")), levels=None)


def _selective_levels(what, name, values):
    try:
        v = [float(x) for x in values]
    except (TypeError, ValueError):
        v = None
    if v is None or len(v) > _lib.SEL_MAX_LEVELS or not all(0.0 <= x <= 1.0 for x in v):
        raise ValueError(f"{what}: {name}={values!r}, expected at most {_lib.SEL_MAX_LEVELS} numbers in [0, 1]")
    return v


def selective_rows(logp, y=None, buf=None, *, score="max_prob", state=None, tau=None):
    """Per row of ``logp`` float32 [N, V] (rows may be padded: ``stride(0) >= V``) the arg-max, whether it is wrong, the confidence
    and whether a threshold accepts the row (``slnlp_selective_rows``, include/slnlp.h), into ``buf`` (``selective_buffers``;
    default a new one, which is returned): ``buf["kappa"]`` float64 [N], ``buf["rows"]`` int32 [N, 4] = (pred, wrong, accepted,
    code).  ``y`` int64 [N] or None: without labels no row is wrong.  ``score``: "max_prob" (the top-class probability, ``topk_rows``'
    bits), "margin" (p(1) - p(2)) or "neg_entropy" (sum p ln p).  ``state``: a calibration state whose beta is read on the device
    (None: beta = 1).  ``tau``: a float64 [4] device tensor whose first entry is the threshold, read on the device; None: nothing
    is accepted.  Runs on the current stream of ``logp``'s device; no host wait."""
    _lib.require_gpu()
    what = "selective_rows"
    N, V, ld = _logp_matrix(what, logp)
    if N > _lib.SEL_MAX_ROWS:
        raise ValueError(f"{what}: {N} rows, the counts are formed for at most {_lib.SEL_MAX_ROWS}")
    if y is not None:
        _labels(what, y, logp.device, N, " or None")
    if score not in _lib.SEL_SCORES:
        raise ValueError(f"{what}: score={score!r}, expected one of {tuple(_lib.SEL_SCORES)}")
    if state is not None:
        _cal_state(what, state, logp.device)
    if tau is not None:
        _conformal_state(what, "tau", tau, logp.device)
    with torch.cuda.device(logp.device):
        if buf is None:
            buf = selective_buffers(N, logp.device)
        _packed_buf(what, buf, f"selective_buffers({N}, {logp.device!r})", (N,), logp.device)
        check(load().slnlp_selective_rows(ptr(logp), ld, ptr(y), N, V, _lib.SEL_SCORES[score], ptr(state), ptr(tau), ptr(buf["kappa"]),
                                          ptr(buf["rows"]), stream_ptr()), what)
    return buf


def selective_counts(buf, risks=(), coverages=()):
    """Per included row of ``buf`` (``selective_rows``' kappa and rows, or ones copied in) how many rows, and how many wrong rows,
    are at least as confident -- ``buf["counts"]`` int32 [N, 2] -- and the summary ``buf["table"]``: n, E, the excluded rows, the
    sum of the selective risks, AURC, coverage at each of ``risks`` and risk at each of ``coverages`` (up to 8 numbers in [0, 1]
    each; ``slnlp_selective_counts``, include/slnlp.h).  Returns the table.  Three queued launches; no host wait."""
    _lib.require_gpu()
    what = "selective_counts"
    _packed_buf(what, buf, "selective_buffers(N, device)", (), None, more=1)
    N, = buf["shape"]
    risks, coverages = _selective_levels(what, "risks", risks), _selective_levels(what, "coverages", coverages)
    r, c = (C.c_double * max(1, len(risks)))(*risks), (C.c_double * max(1, len(coverages)))(*coverages)
    with torch.cuda.device(buf["flat"].device):
        check(load().slnlp_selective_counts(ptr(buf["kappa"]), ptr(buf["rows"]), N, r, len(risks), c, len(coverages), ptr(buf["counts"]),
                                            ptr(buf["table"]), stream_ptr()), what)
    buf["levels"] = (risks, coverages)
    return buf["table"]


def selective_download(buf, counts=True):
    """What a selective-prediction pass hands to the host in ONE device-to-host copy, 32 bytes a row -- the log-probs stay on the
    device: {kappa float64 [N], rows int32 [N, 4], counts int32 [N, 2], table float64 [40 + chunks], risks, coverages} (a piece no
    call has written yet holds whatever the allocation held).  ``counts=False``: kappa and rows alone, 24 bytes a row (what
    ``selective_rows`` by itself writes)."""
    if not counts:
        return buf["packed"].cut("kappa", "rows")
    risks, coverages = buf["levels"] if buf["levels"] is not None else ([], [])
    return {**buf["packed"].cut("table", "counts"), "risks": list(risks), "coverages": list(coverages)}


def error_analysis_buffers(N, V, k, M, device):
    """Every device buffer of one error analysis of an [N, V] set of log-probs -- ``k`` top classes per row (0: none), ``M``
    most-confused pairs -- as slices of ONE int32 allocation, laid out so that whatever is asked for afterwards is one contiguous
    piece of it (``error_analysis_download``):

        confusion [V V + 1] | pairs [M, 3] | counts [3 V + 1] | topk_idx [N, k] | topk_prob float64 [N, k] |
        pred [N] | picked float32 [N] | rank [N] | work

    (one pad entry in front of topk_idx, topk_prob or work where that keeps them 8-byte aligned).  ``score`` = (pred, picked, rank,
    counts) is ``score_rows``' ``out``, ``topk`` = (topk_idx, topk_prob) ``topk_rows``'; the pieces after topk_prob never leave
    the device."""
    what = "error_analysis_buffers"
    N, V = _int_in(what, "N", N, 1, 2 ** 31 - 1), _int_in(what, "V", V, 1, _lib.CONFUSION_MAX_V)
    k, M = _int_in(what, "k", k or 0, 0, min(V, _lib.TOPK_MAX)), _int_in(what, "M", M, 1, _lib.PAIRS_MAX)
    pred, picked, rank, counts = _score_pieces(N, V)
    p = _packed.Packed(torch.int32, (("confusion", torch.int32, V * V + 1, 4), ("pairs", torch.int32, (M, 3), 4), counts,
                                     ("topk_idx", torch.int32, (N, k), 8), ("topk_prob", torch.float64, (N, k), 8), pred, picked, rank,
                                     ("work", torch.uint8, load().slnlp_confusion_pairs_workspace_bytes(V, M), 8)), device)
    buf = _packed_dict(p, (N, V, k, M), at={name: (p.begin(name), p.end(name) - p.begin(name)) for name in p.at})
    if not k:
        buf["topk_idx"] = buf["topk_prob"] = None
    buf.update(score=(buf["pred"], buf["picked"], buf["rank"], buf["counts"]), topk=(buf["topk_idx"], buf["topk_prob"]) if k else None)
    return buf


def error_analysis_download(buf, matrix=True, topk=False):
    """What an error analysis hands to the host, in ONE device-to-host copy of only the pieces asked for: the pairs and the class
    counts always, the V x V matrix with ``matrix``, the top-k lists with ``topk``.  Returns a dict of numpy arrays: ``pairs``
    int32 [M, 3], ``counts`` int64 [3 V + 1], ``confusion`` int64 [V, V] and ``skipped`` (the matrix' tail entry) or None,
    ``topk_idx`` int32 [N, k] and ``topk_prob`` float64 [N, k] or None."""
    import numpy as np
    N, V, k, M = buf["shape"]
    h = buf["packed"].cut("confusion" if matrix else "pairs", "topk_prob" if topk and k else "counts")
    out = {"pairs": h["pairs"], "counts": h["counts"].astype(np.int64), "confusion": None, "skipped": None,
           "topk_idx": h.get("topk_idx"), "topk_prob": h.get("topk_prob")}
    if matrix:
        out["confusion"], out["skipped"] = h["confusion"][:V * V].reshape(V, V).astype(np.int64), int(h["confusion"][V * V])
    return out


def topk_buffers(N, k, device):
    """The two output tensors of ``topk_rows`` -- idx int32 [N, k], prob float64 [N, k] -- as slices of ONE allocation (the
    probabilities first: they need the 8-byte alignment), so ``topk_download`` is one copy."""
    return _packed.Packed(torch.int32, (("prob", torch.float64, (N, k), 8), ("idx", torch.int32, (N, k), 4)), device).views("idx", "prob")


def topk_download(out):
    """``topk_rows``' two tensors as numpy arrays (idx int32 [N, k], prob float64 [N, k]): one device-to-host copy when they are
    ``topk_buffers``' slices of one allocation, two otherwise."""
    return _packed.download(out[::-1], torch.int32)[::-1]


def topk_rows(logp, k, state=None, out=None):
    """The ``k`` most probable classes of every row of ``logp`` float32 [N, V] (rows may be padded: ``stride(0) >= V``) and their
    probabilities under softmax(beta logp) (``slnlp_topk_rows``, include/slnlp.h): ``(idx int32 [N, k], prob float64 [N, k])``,
    device tensors.  The order is the arg-max's (a NaN first, larger values first, equal values by ascending index), so
    ``idx[:, 0]`` is ``score_rows``' ``pred`` and ``prob[:, 0]`` is ``reliability_rows``' conf.  ``state``: a calibration state
    whose beta is read on the device; None: beta = 1.  ``out``: such a pair to fill.  Runs on the current stream of ``logp``'s
    device; no host wait."""
    _lib.require_gpu()
    N, V, ld = _logp_matrix("topk_rows", logp)
    k = _int_in("topk_rows", "k", k, 1, min(V, _lib.TOPK_MAX))
    if state is not None:
        _cal_state("topk_rows", state, logp.device)
    with torch.cuda.device(logp.device):
        if out is None:
            out = topk_buffers(N, k, logp.device)
        idx, prob = out
        for t, dt in ((idx, torch.int32), (prob, torch.float64)):
            _tensor("topk_rows", "out", t, logp.device, dt, (N, k), f"(int32 [{N}, {k}], float64 [{N}, {k}]) on {logp.device}")
        check(load().slnlp_topk_rows(ptr(logp), ld, N, V, k, ptr(state), ptr(idx), ptr(prob), stream_ptr()), "topk_rows")
    return out


def confusion_matrix(pred, y, V, out=None):
    """The confusion matrix of the predictions ``pred`` int32 [N] (``score_rows``' first output) against the labels ``y`` int64
    [N] over ``V`` classes (``slnlp_confusion_matrix``): int32 [V V + 1] on the device -- cell ``y V + pred`` counts the rows with
    that label and that prediction, the last entry the rows whose label or prediction lies outside [0, V).  ``out``: such a tensor
    to fill.  Runs on the current stream of ``pred``'s device; no host wait."""
    _lib.require_gpu()
    if not (pred.is_cuda and pred.dtype == torch.int32 and pred.dim() == 1 and pred.numel() >= 1 and pred.is_contiguous()):
        raise ValueError(f"confusion_matrix: pred must be a contiguous int32 [N] device tensor, got {pred.dtype} {tuple(pred.shape)} on "
                         f"{pred.device}")
    N = pred.numel()
    _labels("confusion_matrix", y, pred.device, N)
    V = _int_in("confusion_matrix", "V", V, 1, _lib.CONFUSION_MAX_V)
    with torch.cuda.device(pred.device):
        if out is None:
            out = torch.empty(V * V + 1, dtype=torch.int32, device=pred.device)
        _tensor("confusion_matrix", "out", out, pred.device, torch.int32, V * V + 1)
        check(load().slnlp_confusion_matrix(ptr(pred), ptr(y), N, V, ptr(out), stream_ptr()), "confusion_matrix")
    return out


def confusion_pairs(counts, V, M, out=None, work=None):
    """The ``M`` most-confused pairs of ``confusion_matrix``'s ``counts`` (``slnlp_confusion_pairs``): int32 [M, 3] on the device,
    rows ``(true, predicted, count)`` over the off-diagonal cells with a count above 0, by count descending, then true class,
    then predicted class ascending; unused rows are (-1, -1, 0).  ``out``: such a tensor to fill; ``work``: a contiguous uint8
    scratch tensor of at least ``slnlp_confusion_pairs_workspace_bytes(V, M)`` bytes (default: a new one).  Runs on the current
    stream of ``counts``' device; no host wait."""
    _lib.require_gpu()
    V = _int_in("confusion_pairs", "V", V, 1, _lib.CONFUSION_MAX_V)
    M = _int_in("confusion_pairs", "M", M, 1, _lib.PAIRS_MAX)
    if not (counts.is_cuda and counts.dtype == torch.int32 and counts.dim() == 1 and counts.numel() in (V * V, V * V + 1)
            and counts.is_contiguous()):
        raise ValueError(f"confusion_pairs: counts must be a contiguous int32 [{V * V + 1}] device tensor, got {counts.dtype} "
                         f"{tuple(counts.shape)} on {counts.device}")
    with torch.cuda.device(counts.device):
        if out is None:
            out = torch.empty(M, 3, dtype=torch.int32, device=counts.device)
        _tensor("confusion_pairs", "out", out, counts.device, torch.int32, (M, 3))
        if work is None:
            work = torch.empty(load().slnlp_confusion_pairs_workspace_bytes(V, M), dtype=torch.uint8, device=counts.device)
        _tensor("confusion_pairs", "work", work, counts.device, torch.uint8, None, f"a contiguous uint8 tensor on {counts.device}")
        check(load().slnlp_confusion_pairs(ptr(counts), V, M, ptr(out), ptr(work), work.numel(), stream_ptr()), "confusion_pairs")
    return out


def error_analysis_rows(logp, y, buf, state=None):
    """One error analysis on the device, into ``error_analysis_buffers``' slices: ``score_rows`` (arg-max and class counts), then
    ``confusion_matrix`` on its ``pred``, ``confusion_pairs`` on the matrix and, when the buffers hold top-k lists,
    ``topk_rows``.  Runs on the current stream of ``logp``'s device; no host wait.  Returns ``buf``."""
    N, V, k, M = buf["shape"]
    score_rows(logp, y, out=buf["score"])
    confusion_matrix(buf["pred"], y, V, out=buf["confusion"])
    confusion_pairs(buf["confusion"], V, M, out=buf["pairs"], work=buf["work"])
    if k:
        topk_rows(logp, k, state=state, out=buf["topk"])
    return buf


def label_audit_buffers(N, V, pairs, device):
    """The device buffer of one label audit of an [N, V] set of log-probs with ``pairs`` likely label swaps, ONE int32 allocation
    laid out as include/slnlp.h states (every piece 8-byte aligned, int32 pieces padded to an even length):

        head int64 [8] | t float64 [V] | s float64 [N] | m float64 [N] | n [V] | joint [V V + 1] | pairs [M, 3] | k [N] | code [N] |
        flags [N] | pred [N] | other float64 [N] | p_pred float64 [N] | work

    What a report needs ends with flags, so ``label_audit_download`` copies one contiguous piece either way."""
    what = "label_audit_buffers"
    N, V = _int_in(what, "N", N, 1, 2 ** 31 - 1), _int_in(what, "V", V, 1, _lib.CONFUSION_MAX_V)
    M = _int_in(what, "pairs", pairs, 1, _lib.PAIRS_MAX)
    reals = lambda name, n: (name, torch.float64, n, 8)
    p = _packed.Packed(torch.int32, (("head", torch.int64, _lib.AUDIT_HEAD_BYTES // 8, 8), reals("t", V), reals("s", N), reals("m", N),
                                     _even_ints("n", V), _even_ints("joint", V * V + 1), _even_ints("pairs", M, 3), _even_ints("k", N),
                                     _even_ints("code", N), _even_ints("flags", N), _even_ints("pred", N), reals("other", N), reals("p_pred", N),
                                     ("work", torch.uint8, load().slnlp_confusion_pairs_workspace_bytes(V, M), 8)), device)
    return {"flat": p.flat, "at": {name: p.begin(name) for name in p.at if name != "head"}, "end": p.flat.numel(), "shape": (N, V, M), "packed": p}


def label_audit_rows(logp, y, buf=None, *, state=None, pairs=20):
    """One confident-learning audit of ``logp`` float32 [N, V] (rows may be padded: ``stride(0) >= V``) against the labels ``y``
    int64 [N] on the device (``slnlp_label_audit``, include/slnlp.h): per class the threshold t_c (the mean self-confidence of its
    rows), per row the class it is confidently predicted as, the confident joint and its ``pairs`` largest off-diagonal cells,
    into ``buf`` (``label_audit_buffers``; default a new one, which is returned).  ``state``: a calibration state whose beta is read
    on the device (None: beta = 1).  Eight queued launches on the current stream of ``logp``'s device; no host wait."""
    _lib.require_gpu()
    what = "label_audit_rows"
    N, V, ld = _logp_matrix(what, logp)
    if V > _lib.CONFUSION_MAX_V:
        raise ValueError(f"{what}: {V} classes, the confident joint is formed for at most {_lib.CONFUSION_MAX_V}")
    _labels(what, y, logp.device, N)
    if state is not None:
        _cal_state(what, state, logp.device)
    with torch.cuda.device(logp.device):
        if buf is None:
            buf = label_audit_buffers(N, V, pairs, logp.device)
        _packed_buf(what, buf, f"label_audit_buffers({N}, {V}, pairs, {logp.device!r})", (N, V), logp.device, more=1)
        check(load().slnlp_label_audit(ptr(logp), ld, ptr(y), N, V, ptr(state), buf["shape"][2], ptr(buf["flat"]),
                                       buf["flat"].numel() * 4, stream_ptr()), what)
    return buf


def label_audit_download(buf, per_row=False):
    """What a label audit hands to the host in ONE device-to-host copy -- the log-probs stay on the device: {head int64 [8] =
    (usable rows, bad_labels, nan_rows, unconfident, issues, argmax_disagrees, 0, 0), t float64 [V], n int32 [V], joint int64
    [V, V], overflow, pairs int32 [M, 3], k / code / flags int32 [N], s / m float64 [N]}: what ``metrics.label_audit_report`` reads.
    ``per_row=True`` extends the copy by pred int32 [N], other and p_pred float64 [N]."""
    import numpy as np
    V = buf["shape"][1]
    out = buf["packed"].cut("head", "p_pred" if per_row else "flags")
    out.update(joint=out["joint"][:V * V].reshape(V, V).astype(np.int64), overflow=int(out["joint"][V * V]))
    return out


TRAIN_DYNAMICS_ROW_INTS = ("visits", "correct_visits", "epochs_seen", "epochs_correct", "forgetting", "first_learned", "last")


def train_dynamics_buffers(N, n_visit, device):
    """The device buffer of a fit's training dynamics over ``N`` dataset rows, fed ``n_visit`` visit positions per epoch: ONE int32
    allocation laid out as include/slnlp.h states (every piece 8-byte aligned, int32 pieces padded to an even length) -- the state

        head int64 [8] | sum_q int64 [N] | sum_q2 int64 [N] | sum_mq int64 [N] | visits [N] | correct_visits [N] | epochs_seen [N] |
        epochs_correct [N] | forgetting [N] | first_learned [N] | last [N] | v_e [N] | c_e [N]

    and behind it the per-visit scratch of one epoch: ``q int64 [n_visit] | mq int64 [n_visit] | code | correct | pred [n_visit]``.
    What a report needs ends with last, so ``train_dynamics_download`` copies one contiguous piece; ``state_bytes`` is where the
    scratch begins.  (The unsigned pieces are held as signed ones: below the visit limit no value reaches a sign bit.)  The state is
    NOT zeroed: ``train_dynamics_reset`` does that."""
    what = "train_dynamics_buffers"
    N, n = _int_in(what, "N", N, 1, 2 ** 31 - 1), _int_in(what, "n_visit", n_visit, 1, 2 ** 31 - 1)
    longs = lambda name, k: (name, torch.int64, k, 8)
    p = _packed.Packed(torch.int32, (("head", torch.int64, _lib.DYN_HEAD_BYTES // 8, 8), longs("sum_q", N), longs("sum_q2", N), longs("sum_mq", N),
                                     *(_even_ints(name, N) for name in TRAIN_DYNAMICS_ROW_INTS), _even_ints("v_e", N), _even_ints("c_e", N),
                                     longs("q", n), longs("mq", n), _even_ints("code", n), _even_ints("correct", n), _even_ints("pred", n)), device)
    state_bytes = p.at["q"][0]
    if state_bytes != load().slnlp_train_dynamics_state_bytes(N):
        raise RuntimeError(f"{what}: the state of {N} rows is laid out in {state_bytes} bytes here and in "
                           f"{load().slnlp_train_dynamics_state_bytes(N)} by the library")
    return _packed_dict(p, (N, n), state_bytes=state_bytes)


def _dyn_buf(what, buf, device=None):
    _packed_buf(what, buf, "train_dynamics_buffers(N, n_visit, device)", (), device, more=2)
    return buf["flat"], buf["state_bytes"], buf["flat"].numel() * 4 - buf["state_bytes"]


def train_dynamics_reset(buf):
    """Zero the state of ``train_dynamics_buffers`` (first_learned and last: -1) with one launch of the library's own
    (``slnlp_train_dynamics_reset``) on the current stream of the buffer's device; no host wait.  Returns ``buf``."""
    _lib.require_gpu()
    what = "train_dynamics_reset"
    flat, state_bytes, _ = _dyn_buf(what, buf)
    with torch.cuda.device(flat.device):
        check(load().slnlp_train_dynamics_reset(ptr(flat), state_bytes, buf["shape"][0], stream_ptr()), what)
    return buf


def train_dynamics_epoch(logp, y, order, epoch, buf):
    """Fold ONE epoch's train log-probs into the training-dynamics state ``buf`` (``train_dynamics_buffers``):
    ``slnlp_train_dynamics_epoch``, include/slnlp.h.  ``logp`` float32 [n_visit, V] in visit order (rows may be padded:
    ``stride(0) >= V``), ``y`` int64 [n_visit] the labels in visit order, ``order`` int64 [n_visit] the dataset row of every visit
    or None (visit i is row i), ``epoch`` >= 1 its number.  Two queued launches on the current stream of ``logp``'s device; no host
    wait.  Returns ``buf``, whose per-visit scratch holds this epoch's values until the next call."""
    _lib.require_gpu()
    what = "train_dynamics_epoch"
    n, V, ld = _logp_matrix(what, logp)
    _labels(what, y, logp.device, n)
    if order is not None:
        _tensor(what, "order", order, logp.device, torch.int64, n, f"a contiguous int64 [{n}] tensor on {logp.device} or None")
    epoch = _int_in(what, "epoch", epoch, 1, 2 ** 31 - 1)
    flat, state_bytes, visits_bytes = _dyn_buf(what, buf, logp.device)
    if buf["shape"][1] != n:
        raise ValueError(f"{what}: buf was made for {buf['shape'][1]} visits per epoch, logp has {n} rows")
    with torch.cuda.device(logp.device):
        check(load().slnlp_train_dynamics_epoch(ptr(logp), ld, ptr(y), ptr(order), n, V, buf["shape"][0], epoch, ptr(flat), state_bytes,
                                                ptr(flat) + state_bytes, visits_bytes, stream_ptr()), what)
    return buf


def train_dynamics_download(buf, per_visit=False):
    """What the training dynamics hand to the host in ONE device-to-host copy: {head int64 [8] = (epochs, usable visits, bad_labels,
    nan_rows, bad_rows, rows seen, overflow, 0), sum_q / sum_q2 / sum_mq int64 [N], visits / correct_visits / epochs_seen /
    epochs_correct / forgetting / first_learned / last int32 [N]}: what ``metrics.train_dynamics_report`` reads.
    ``per_visit=True`` extends the copy through the last epoch's per-visit scratch: q / mq int64, code / correct / pred int32
    [n_visit] (and the fold's v_e / c_e, which are 0 between epochs)."""
    _dyn_buf("train_dynamics_download", buf)
    return buf["packed"].cut("head", "pred" if per_visit else "last")


def occlusion_variants(lengths, S, by, width=1, stride=1, bins=8, n_fields=None):
    """The variant table of an occlusion attribution over rows of ``lengths`` (host integers [N]) padded to ``S`` positions
    (include/slnlp.h): ``(variants int32 [M, 3] = (row, unit, bin) sorted by (row, unit), row_start int32 [N + 1], n_bins)``.
    With len = clamp(L[i], 0, S): ``by`` "mask" / "drop": the units are the windows [u stride, min(u stride + width, len)) with
    u stride < len -- a row of length 0 has none -- and the bin is the relative position of the window's centre,
    min(bins - 1, (bins (lo + hi)) // (2 len)) in integers; ``n_bins = bins``.  ``by`` "field": one unit per field u in
    0..n_fields - 1 for a row with len >= 1, the bin is u and ``n_bins = n_fields``.  ``bins`` and ``n_fields`` lie in 1..64,
    ``width`` and ``stride`` in 1..S, M in 0..2^31 - 1.  Host arithmetic: no GPU is needed."""
    import numpy as np
    what = "occlusion_variants"
    L = np.asarray(lengths)
    if L.ndim != 1 or L.dtype.kind not in "iu":
        raise ValueError(f"{what}: lengths must be one dimension of integers, got {L.dtype} {L.shape}")
    S = _int_in(what, "S", S, 1, 2 ** 31 - 1)
    if by not in ("mask", "drop", "field"):
        raise ValueError(f"{what}: by={by!r}, expected 'mask', 'drop' or 'field'")
    ln = np.clip(L.astype(np.int64), 0, S)
    if by == "field":
        n_bins = _int_in(what, "n_fields", n_fields, 1, _lib.ATTR_MAX_BINS)
        counts = np.where(ln >= 1, n_bins, 0)
    else:
        width, stride = _int_in(what, "width", width, 1, S), _int_in(what, "stride", stride, 1, S)
        n_bins = _int_in(what, "bins", bins, 1, _lib.ATTR_MAX_BINS)
        counts = (ln + stride - 1) // stride                 # the units u with u stride < len
    row_start = np.zeros(ln.size + 1, dtype=np.int64)
    np.cumsum(counts, out=row_start[1:])
    M = int(row_start[-1])
    if M > 2 ** 31 - 1:
        raise ValueError(f"{what}: {M} variants, at most {2 ** 31 - 1} fit a table")
    rows = np.repeat(np.arange(ln.size, dtype=np.int64), counts)
    unit = np.arange(M, dtype=np.int64) - row_start[rows]
    if by == "field":
        bin_ = unit
    else:
        lo = unit * stride
        hi = np.minimum(lo + width, ln[rows])
        bin_ = np.minimum(n_bins - 1, (n_bins * (lo + hi)) // (2 * ln[rows]))
    return np.stack([rows, unit, bin_], axis=1).astype(np.int32).reshape(M, 3), row_start.astype(np.int32), n_bins


def occlude_rows(X, L, y, variants, kind, *, width=1, stride=1, pad=1, unk=0, sub=None, out=None):
    """The variants' inputs, built on the device (``slnlp_occlude_rows``, csrc/attribution.hip): for each entry (row, unit, .) of
    ``variants`` int32 [m, 3] -- a device tensor, or a slice of the table's rows -- a copy of row ``row`` of ``X`` int64 [n, S] /
    ``L`` / ``y`` int64 [n] with the unit hidden: ``kind`` "mask" (the window becomes ``unk``), "drop" (the window is deleted and
    the rest closes up; a window over the whole row is masked) or "substitute" (every token goes through ``sub`` int64 [Vx, F],
    column ``unit``).  Returns ``(X_out [m, S], L_out [m], y_out [m])``; ``out``: that triple to fill.  One launch on the current
    stream of ``X``'s device; no host wait."""
    _lib.require_gpu()
    what = "occlude_rows"
    if kind not in _lib.OCCLUDE_KINDS:
        raise ValueError(f"{what}: kind={kind!r}, expected one of {_lib.OCCLUDE_KINDS}")
    if not (X.is_cuda and X.dtype == torch.int64 and X.dim() == 2 and X.is_contiguous()):
        raise ValueError(f"{what}: X must be a contiguous int64 [n, S] device tensor")
    n, S = int(X.shape[0]), int(X.shape[1])
    _tensor(what, "L", L, X.device, torch.int64, n)
    _tensor(what, "y", y, X.device, torch.int64, n)
    if not (variants.device == X.device and variants.dtype == torch.int32 and variants.dim() == 2 and variants.shape[1] == 3
            and variants.is_contiguous() and variants.shape[0] >= 1):
        raise ValueError(f"{what}: variants must be a contiguous int32 [m >= 1, 3] tensor on {X.device}")
    m = int(variants.shape[0])
    Vx = F = 0
    if kind == "substitute":
        if not (torch.is_tensor(sub) and sub.device == X.device and sub.dtype == torch.int64 and sub.dim() == 2 and sub.is_contiguous()):
            raise ValueError(f"{what}: substitute needs sub, a contiguous int64 [Vx, F] tensor on {X.device}")
        Vx, F = int(sub.shape[0]), int(sub.shape[1])
    else:
        sub = None
    with torch.cuda.device(X.device):
        if out is None:
            out = (torch.empty(m, S, dtype=torch.int64, device=X.device), torch.empty(m, dtype=torch.int64, device=X.device),
                   torch.empty(m, dtype=torch.int64, device=X.device))
        Xo, Lo, yo = out
        _tensor(what, "X_out", Xo, X.device, torch.int64, (m, S))
        _tensor(what, "L_out", Lo, X.device, torch.int64, m)
        _tensor(what, "y_out", yo, X.device, torch.int64, m)
        check(load().slnlp_occlude_rows(ptr(X), ptr(L), ptr(y), n, S, ptr(variants), m, _lib.OCCLUDE_KINDS.index(kind), int(width), int(stride),
                                        int(pad), int(unk), ptr(sub), Vx, F, ptr(Xo), ptr(Lo), ptr(yo), stream_ptr()), what)
    return Xo, Lo, yo


def attribution_buffers(N, V, variants, row_start, n_bins, device):
    """The device buffer of one attribution of N rows of V classes under a variant table (``occlusion_variants``' host arrays,
    uploaded here), ONE int32 allocation, every piece 8-byte aligned (int32 pieces padded to an even length):

        head int64 [8] | table_i int64 [V, n_bins, 3] | table_d float64 [V, n_bins, 2] | rows_d float64 [N, 4] | rows_i [N, 6] |
        vals float64 [M, 3] | ints [M, 2] | cell [M] | variants [M, 3] | row_start [N + 1]

    What a report needs ends with rows_i and the per-variant values follow, so ``attribution_download`` copies one contiguous
    piece either way.  ``buf[name]`` is the piece as a tensor view."""
    import numpy as np
    what = "attribution_buffers"
    N, V = _int_in(what, "N", N, 1, 2 ** 31 - 1), _int_in(what, "V", V, 1, _lib.CONFUSION_MAX_V)
    nb = _int_in(what, "n_bins", n_bins, 1, _lib.ATTR_MAX_BINS)
    variants = np.ascontiguousarray(variants, dtype=np.int32)
    row_start = np.ascontiguousarray(row_start, dtype=np.int32)
    if variants.ndim != 2 or variants.shape[1] != 3 or not 1 <= variants.shape[0] <= (2 ** 31 - 1) // 3 or row_start.shape != (N + 1,):
        raise ValueError(f"{what}: variants int32 [M, 3] with M in 1..{(2 ** 31 - 1) // 3} and row_start int32 [{N + 1}] expected, got "
                         f"{variants.shape} and {row_start.shape}")
    M = int(variants.shape[0])
    p = _packed.Packed(torch.int32, (("head", torch.int64, _lib.ATTR_HEAD_BYTES // 8, 8), ("table_i", torch.int64, (V, nb, 3), 8),
                                     ("table_d", torch.float64, (V, nb, 2), 8), ("rows_d", torch.float64, (N, 4), 8),
                                     _even_ints("rows_i", N, 6), ("vals", torch.float64, (M, 3), 8), _even_ints("ints", M, 2),
                                     _even_ints("cell", M), _even_ints("variants", M, 3), _even_ints("row_start", N + 1)), device)
    buf = _packed_dict(p, (N, V, M, nb), shaped=False, at={name: p.begin(name) for name in p.at}, end=p.flat.numel())
    buf["variants"] = buf["variants"].view(M, 3)             # (the other pieces in one dimension, as the kernels index them)
    buf["variants"].copy_(torch.from_numpy(variants))
    buf["row_start"].copy_(torch.from_numpy(row_start))
    return buf


def _attribution_args(what, base, y, buf, target, state):
    N, V, ld = _logp_matrix(what, base)
    _packed_buf(what, buf, f"attribution_buffers({N}, {V}, ...) on {base.device}", (N, V), base.device, more=2)
    if target not in _lib.ATTR_TARGETS:
        raise ValueError(f"{what}: target={target!r}, expected one of {_lib.ATTR_TARGETS}")
    if y is not None or target == "label":
        if y is None:
            raise ValueError(f"{what}: target 'label' needs the labels y")
        _labels(what, y, base.device, N)
    if state is not None:
        _cal_state(what, state, base.device)
    return N, V, ld


def attribution_rows(base, var, y, buf, off, *, target="label", state=None):
    """Judge the variant rows ``var`` float32 [m, V] -- variants ``off .. off + m - 1`` of ``buf``'s table -- against their base
    rows in ``base`` float32 [N, V] (``slnlp_attribution_rows``, include/slnlp.h): drop, dp and kl into ``buf["vals"]``, the
    variant's arg-max and code into ``buf["ints"]``.  ``y``: int64 [N] labels (may be None with ``target="pred"``, the base
    row's arg-max); ``state``: a calibration state whose beta is read on the device (None: beta = 1).  One launch on the current
    stream of ``base``'s device; no host wait.  Returns ``buf``."""
    _lib.require_gpu()
    what = "attribution_rows"
    N, V, ld = _attribution_args(what, base, y, buf, target, state)
    m, Vv, ld_v = _logp_matrix(what + " (var)", var)
    M = buf["shape"][2]
    off = _int_in(what, "off", off, 0, M)
    if Vv != V or var.device != base.device or off + m > M:
        raise ValueError(f"{what}: var must hold at most {M - off} rows of {V} classes on {base.device} at off={off}, got {tuple(var.shape)}")
    with torch.cuda.device(base.device):
        check(load().slnlp_attribution_rows(ptr(base), ld, ptr(var), ld_v, ptr(y), ptr(buf["variants"]), N, m, V, _lib.ATTR_TARGETS.index(target),
                                            ptr(state), off, ptr(buf["vals"]), ptr(buf["ints"]), stream_ptr()), what)
    return buf


def attribution_summary(base, y, buf, *, target="label", state=None):
    """Reduce ``buf``'s finished table on the device (``slnlp_attribution_summary``): per row the base arg-max, the target, its
    log-probability, the usable variants, the flips, top_unit / top_drop, min_drop and sum_drop; the [V, n_bins] table keyed by
    (target class, bin); the head.  ``base``, ``y``, ``target`` and ``state`` as for ``attribution_rows``.  Four queued launches on
    the current stream of ``base``'s device; no host wait.  Returns ``buf``."""
    _lib.require_gpu()
    what = "attribution_summary"
    N, V, ld = _attribution_args(what, base, y, buf, target, state)
    M, nb = buf["shape"][2:]
    with torch.cuda.device(base.device):
        check(load().slnlp_attribution_summary(ptr(base), ld, ptr(y), ptr(buf["variants"]), ptr(buf["row_start"]), N, M, V, nb,
                                               _lib.ATTR_TARGETS.index(target), ptr(state), ptr(buf["vals"]), ptr(buf["ints"]), ptr(buf["cell"]),
                                               ptr(buf["head"]), ptr(buf["table_i"]), ptr(buf["table_d"]), ptr(buf["rows_i"]), ptr(buf["rows_d"]),
                                               stream_ptr()), what)
    return buf


def attribution_download(buf, per_variant=False):
    """What an attribution hands to the host in ONE device-to-host copy -- the log-probs stay on the device: {head int64 [8] =
    (usable, bad_labels, nonfinite, invalid, flips, 0, 0, 0), table_i int64 [V, n_bins, 3] = (count, flips, nonfinite), table_d
    float64 [V, n_bins, 2] = (sum drop, sum kl), rows_d float64 [N, 4] = (base log-prob of the target, top_drop, min_drop,
    sum_drop), rows_i int32 [N, 6] = (base_pred, target, code, units, flips, top_unit)}: what ``metrics.attribution_report`` reads.
    ``per_variant=True`` extends the copy by vals float64 [M, 3] = (drop, dp, kl) and ints int32 [M, 2] = (arg-max, code)."""
    return buf["packed"].cut("head", "ints" if per_variant else "rows_i")


def _edit_side(what, side, X, L):
    """One side of the edit-distance entry points: ``X`` int64 [n, S] with unit column stride (rows may be padded: ``stride(0) >=
    S``), ``L`` int64 [n] on its device -> (n, row stride)"""
    if not (torch.is_tensor(X) and X.is_cuda and X.dtype == torch.int64 and X.dim() == 2 and X.shape[0] >= 1 and X.shape[1] >= 1
            and (X.stride(1) == 1 or X.shape[1] == 1) and X.stride(0) >= X.shape[1]):
        raise ValueError(f"{what}: the {side} rows must be an int64 [n >= 1, S >= 1] device tensor with unit column stride")
    n = int(X.shape[0])
    if not torch.is_tensor(L):
        raise ValueError(f"{what}: the {side} lengths must be a contiguous int64 [{n}] tensor on {X.device}")
    _tensor(what, f"the {side} lengths", L, X.device, torch.int64, n)
    return n, int(X.stride(0)) if n > 1 else max(int(X.shape[1]), int(X.stride(0)))


def _edit_pairs(what, nq, nr, width):
    says = "one byte" if width == 1 else "two bytes"
    if nq * nr > _lib.EDIT_MAX_PAIRS:
        raise ValueError(f"{what}: {nq} x {nr} pairs, at most {_lib.EDIT_MAX_PAIRS} ({says} each) are formed per call: pass the queries in chunks")


def _knn_sides(what, Xq, Lq, Xr, Lr):
    """Both sides of a neighbour search, the references on the queries' device -> (nq, ldq, nr, ldr, device)"""
    nq, ldq = _edit_side(what, "query", Xq, Lq)
    if not (torch.is_tensor(Xr) and Xr.device == Xq.device):
        raise ValueError(f"{what}: the reference rows must be a tensor on {Xq.device}")
    nr, ldr = _edit_side(what, "reference", Xr, Lr)
    return nq, ldq, nr, ldr, Xq.device


def _knn_distances(what, dtype, says, Xq, Lq, Xr, Lr, out, metric):
    """The body of the three ``*_distances``: sides, pairs (refused as ``says`` bytes each), then ``metric(device)`` -> (entry point,
    its arguments between ``nr`` and the matrix) with the metric's own checks, then ``out`` of ``dtype`` and the call"""
    _lib.require_gpu()
    nq, ldq, nr, ldr, dev = _knn_sides(what, Xq, Lq, Xr, Lr)
    _edit_pairs(what, nq, nr, says)
    entry, args = metric(dev)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(nq, nr, dtype=dtype, device=dev)
        _tensor(what, "out", out, dev, dtype, (nq, nr))
        check(entry(ptr(Xq), ldq, ptr(Lq), nq, ptr(Xr), ldr, ptr(Lr), nr, *args, ptr(out), stream_ptr()), what)
    return out


def _knn_rows(what, width, says, Xq, Lq, Xr, Lr, k, exclude, buf, scratch, metric):
    """The body of the three ``*_knn_rows`` behind their integer checks: sides, pairs (refused as ``says`` bytes each), then
    ``metric(device)`` -> (entry point, its arguments between ``nr`` and ``exclude``, radius) with the metric's own checks, then
    ``exclude``, ``buf``, the scratch of ``width`` bytes a pair and the call"""
    _lib.require_gpu()
    nq, ldq, nr, ldr, dev = _knn_sides(what, Xq, Lq, Xr, Lr)
    _edit_pairs(what, nq, nr, says)
    entry, args, radius = metric(dev)
    if exclude is not None:
        _tensor(what, "exclude", exclude, dev, torch.int64, nq, f"a contiguous int64 [{nq}] tensor on {dev} or None")
    with torch.cuda.device(dev):
        if buf is None:
            buf = edit_knn_buffers(nq, k, dev)
        _packed_buf(what, buf, f"edit_knn_buffers({nq}, {k}, device) on {dev}", (nq, k), dev)
        if scratch is None:
            scratch = torch.empty(width * nq * nr, dtype=torch.uint8, device=dev)
        _tensor(what, "scratch", scratch, dev, torch.uint8, None, f"a contiguous uint8 [>= {width * nq * nr}] tensor on {dev}")
        check(entry(ptr(Xq), ldq, ptr(Lq), nq, ptr(Xr), ldr, ptr(Lr), nr, *args, ptr(exclude), k, radius, ptr(scratch), scratch.numel(),
                    ptr(buf["head"]), ptr(buf["rows"]), ptr(buf["nbr"]), stream_ptr()), what)
    return buf


def _knn_logp(what, entry, buf, Lq, Lr, yr, prior, extra, weights, tau, normalize, lam, out):
    """The body of the three ``*_knn_logp``; ``extra``: None, or (name, value, lowest, highest) of the one integer that the entry
    point takes behind ``V``, checked where it always was (behind ``buf``)"""
    _packed_buf(what, buf, "edit_knn_buffers(nq, k, device)", (), None, more=2)
    nq, k = buf["shape"]
    dev = buf["flat"].device
    extra = () if extra is None else (_int_in(what, *extra),)
    if weights not in _lib.EDIT_WEIGHTS:
        raise ValueError(f"{what}: weights={weights!r}, expected one of {_lib.EDIT_WEIGHTS}")
    tau, lam = _positive(what, "tau", tau), _positive(what, "lam", lam)
    _lib.require_gpu()
    for name, t in (("Lq", Lq), ("Lr", Lr), ("yr", yr), ("prior", prior)):
        if not torch.is_tensor(t):
            raise ValueError(f"{what}: {name} must be a tensor on {dev}")
    _tensor(what, "Lq", Lq, dev, torch.int64, nq)
    _tensor(what, "Lr", Lr, dev, torch.int64, None)
    nr = int(Lr.shape[0])
    _tensor(what, "yr", yr, dev, torch.int64, nr)
    _tensor(what, "prior", prior, dev, torch.float64, None)
    V = int(prior.shape[0])
    if nr < 1 or V < 1:
        raise ValueError(f"{what}: {nr} references and {V} classes: at least one of each")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(nq, V, dtype=torch.float32, device=dev)
        if out.device != dev or tuple(out.shape) != (nq, V):
            raise ValueError(f"{what}: out must be a float32 [{nq}, {V}] tensor on {dev}")
        ld = _logp_matrix(f"{what} (out)", out)[2]
        check(getattr(load(), entry)(ptr(buf["nbr"]), ptr(buf["rows"]), ptr(Lq), ptr(Lr), ptr(yr), nq, nr, k, V, *extra, _lib.EDIT_WEIGHTS.index(weights),
                                     tau, int(bool(normalize)), lam, ptr(prior), ptr(out), ld, ptr(buf["head"]), stream_ptr()), what)
    return out


def edit_distances(Xq, Lq, Xr, Lr, out=None):
    """The unit-cost Levenshtein distance of every (query, reference) pair (``slnlp_edit_distances``, csrc/edit_knn.hip): ``Xq`` int64
    [nq, S] / ``Lq`` int64 [nq] against ``Xr`` int64 [nr, S'] / ``Lr`` int64 [nr] -> uint8 [nq, nr]; 255 where either row's length
    lies outside 0..64 (or beyond its row).  Only the first L tokens of a row are read.  ``out``: the matrix to fill.  One launch on
    the current stream of ``Xq``'s device; no host wait."""
    return _knn_distances("edit_distances", torch.uint8, 1, Xq, Lq, Xr, Lr, out, lambda dev: (load().slnlp_edit_distances, ()))


def edit_knn_buffers(nq, k, device):
    """The outputs of ``edit_knn_rows`` for ``nq`` queries and ``k`` neighbours as slices of ONE int32 allocation, so that
    ``edit_knn_download`` is one copy:

        head int64 [8] | rows int32 [nq, 4] | nbr int32 [nq, k, 2]"""
    what = "edit_knn_buffers"
    nq, k = _int_in(what, "nq", nq, 1, _lib.EDIT_MAX_ROWS), _int_in(what, "k", k, 1, _lib.EDIT_MAX_K)
    p = _packed.Packed(torch.int32, (("head", torch.int64, _lib.EDIT_HEAD_BYTES // 8, 8), ("rows", torch.int32, (nq, 4), 8),
                                     ("nbr", torch.int32, (nq, k, 2), 8)), device)
    return _packed_dict(p, (nq, k))




def edit_knn_rows(Xq, Lq, Xr, Lr, k, *, radius=0, exclude=None, buf=None, scratch=None):
    """The ``k`` (1..64) nearest references of every query under Levenshtein distance (``slnlp_edit_knn_rows``): per query the
    usable references of smallest distance ordered by (distance, reference index) -- ties at the k-th distance go to the lower
    index -- into ``buf`` (``edit_knn_buffers(nq, k, device)``; None: a new one).  ``exclude``: int64 [nq] on the device, the one
    reference index query i skips (leave-one-out; -1: none), or None.  ``radius`` (0..64): ``rows[:, 1]`` counts the usable
    references within it.  ``scratch``: a uint8 tensor of at least nq nr elements to hold the distances (None: a new one; it holds
    the uint8 [nq, nr] matrix afterwards).  Three queued launches on the current stream of ``Xq``'s device; no host wait.
    Returns ``buf``."""
    what = "edit_knn_rows"
    k, radius = _int_in(what, "k", k, 1, _lib.EDIT_MAX_K), _int_in(what, "radius", radius, 0, _lib.EDIT_MAX_LEN)
    return _knn_rows(what, 1, 1, Xq, Lq, Xr, Lr, k, exclude, buf, scratch, lambda dev: (load().slnlp_edit_knn_rows, (), radius))


def edit_knn_logp(buf, Lq, Lr, yr, prior, *, weights="distance", tau=1.0, normalize=True, lam=1.0, out=None):
    """The neighbours of ``buf`` (``edit_knn_rows``) as float32 log-probs [nq, V] (``slnlp_edit_knn_logp``, include/slnlp.h states the
    vote): ``Lq`` int64 [nq] and ``Lr`` / ``yr`` int64 [nr] the lengths and the references' labels, ``prior`` float64 [V] on the
    device; ``weights`` "uniform" or "distance" (w = exp(-d / (tau n)), n = max(Lq, Lr, 1) when ``normalize``), ``lam`` > 0 the
    weight of the prior.  A flagged query gets a row of NaN; ``buf["head"][2]`` counts the neighbours whose label lies outside the
    V classes.  ``out``: a float32 [nq, V] tensor to fill (rows may be padded).  Two queued launches on the current stream of
    ``buf``'s device; no host wait.  Returns ``out``."""
    return _knn_logp("edit_knn_logp", "slnlp_edit_knn_logp", buf, Lq, Lr, yr, prior, None, weights, tau, normalize, lam, out)


def edit_knn_download(buf, neighbours=True):
    """What a neighbour search hands to the host in ONE device-to-host copy: {head int64 [8] = (flagged queries, flagged references,
    neighbours with a label outside the classes, 0, ...), rows int32 [nq, 4] = (found, references within the radius, nearest
    distance or -1, code bits: 1 the query's length is outside 0..64, 2 its ``exclude`` entry names no reference), nbr int32 [nq, k,
    2] = (distance, reference index), (-1, -1) past found}; ``neighbours=False`` stops behind rows."""
    _packed_buf("edit_knn_download", buf, "edit_knn_buffers(nq, k, device)", (), None, more=2)
    return buf["packed"].cut("head", "nbr" if neighbours else "rows")




def edit_long_distances(Xq, Lq, Xr, Lr, *, max_len, out=None):
    """``edit_distances`` for rows of up to ``max_len`` (1..512) frames (``slnlp_edit_long_distances``, csrc/edit_long.hip: Myers'
    recurrence in its multi-word form) -> uint16 [nq, nr]; 65535 where either row's length lies outside 0..max_len (or beyond its
    row): a longer row is refused, never truncated.  Where both apply the values are ``edit_distances``'s.  ``out``: the matrix to
    fill.  One launch on the current stream of ``Xq``'s device; no host wait."""
    what = "edit_long_distances"
    max_len = _int_in(what, "max_len", max_len, -2 ** 63, 2 ** 63 - 1)          # the library holds it to 1..512
    return _knn_distances(what, torch.uint16, 2, Xq, Lq, Xr, Lr, out, lambda dev: (load().slnlp_edit_long_distances, (max_len,)))


def edit_long_knn_rows(Xq, Lq, Xr, Lr, k, *, max_len, radius=0, exclude=None, buf=None, scratch=None):
    """``edit_knn_rows`` for rows of up to ``max_len`` (1..512) frames (``slnlp_edit_long_knn_rows``): the same selection into the
    same ``buf`` (``edit_knn_buffers(nq, k, device)``; None: a new one), ``radius`` in 0..max_len; the code bit 1 of ``rows[:, 3]``
    says that the query's length lies outside 0..max_len.  ``scratch``: a uint8 tensor of at least 2 nq nr bytes, 2-byte aligned
    (None: a new one; it holds the uint16 [nq, nr] matrix afterwards).  Three queued launches on the current stream of ``Xq``'s
    device; no host wait.  Returns ``buf``."""
    what = "edit_long_knn_rows"
    max_len = _int_in(what, "max_len", max_len, -2 ** 63, 2 ** 63 - 1)          # the library holds it to 1..512 and the radius to 0..max_len
    k, radius = _int_in(what, "k", k, 1, _lib.EDIT_MAX_K), _int_in(what, "radius", radius, -2 ** 63, 2 ** 63 - 1)
    return _knn_rows(what, 2, 2, Xq, Lq, Xr, Lr, k, exclude, buf, scratch, lambda dev: (load().slnlp_edit_long_knn_rows, (max_len,), radius))


def edit_long_knn_logp(buf, Lq, Lr, yr, prior, *, max_len, weights="distance", tau=1.0, normalize=True, lam=1.0, out=None):
    """``edit_knn_logp`` for the neighbours of ``edit_long_knn_rows`` (``slnlp_edit_long_knn_logp``): the same vote, operation for
    operation, but a neighbour is listed up to the distance ``max_len`` (1..512) where ``edit_knn_logp`` lists none beyond 64.  Two
    queued launches on the current stream of ``buf``'s device; no host wait.  Returns ``out``."""
    return _knn_logp("edit_long_knn_logp", "slnlp_edit_long_knn_logp", buf, Lq, Lr, yr, prior, ("max_len", max_len, -2 ** 63, 2 ** 63 - 1),
                     weights, tau, normalize, lam, out)             # the library holds max_len to 1..512


def _field_table(what, codes, gap, dev):
    """The code table of the weighted edit distance: ``codes`` a contiguous int32 [Vt >= 1, F in 1..16] tensor on ``dev``, ``gap``
    an integer in 1..F (None: F) -> (Vt, F, gap)"""
    if not (torch.is_tensor(codes) and codes.dtype == torch.int32 and codes.dim() == 2 and codes.shape[0] >= 1
            and 1 <= codes.shape[1] <= _lib.FIELD_MAX_FIELDS and codes.is_contiguous() and codes.device == dev):
        raise ValueError(f"{what}: codes must be a contiguous int32 [Vt >= 1, F in 1..{_lib.FIELD_MAX_FIELDS}] tensor on {dev}")
    Vt, F = int(codes.shape[0]), int(codes.shape[1])
    return Vt, F, _int_in(what, "gap", F if gap is None else gap, 1, F)


def _field_weights(what, field_weights, F, gap):
    """The per-field weights of the weighted metric checked on the host: ``field_weights`` a sequence of F integers in 0..16 whose
    sum W lies in 1..16, ``gap`` an integer in 1..W (None: W) -> (ctypes int32 [F] array, W, gap); anything else raises ValueError"""
    try:
        w = list(field_weights)
    except TypeError:
        w = None
    whole = lambda v: isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if w is None or len(w) != F or not all(whole(v) and 0 <= v <= _lib.FIELD_MAX_WEIGHT for v in w):
        raise ValueError(f"{what}: field_weights={field_weights!r}, expected {F} integers in 0..{_lib.FIELD_MAX_WEIGHT} (one per field)")
    W = int(sum(int(v) for v in w))
    if not 1 <= W <= _lib.FIELD_MAX_WEIGHT:
        raise ValueError(f"{what}: field_weights={tuple(int(v) for v in w)} sum to W={W}, expected 1..{_lib.FIELD_MAX_WEIGHT}")
    return (C.c_int32 * F)(*(int(v) for v in w)), W, _int_in(what, "gap", W if gap is None else gap, 1, W)



def _field_metric(what, codes, gap, field_weights, dev):
    """The table, the weights and the gap of either field metric checked -> (arguments of the entry point behind ``nr``, unit: F or
    W, "_w" where the weighted entry point takes them)"""
    if field_weights is None:
        Vt, F, gap = _field_table(what, codes, gap, dev)
        return (ptr(codes), Vt, F, gap), F, ""
    Vt, F, _ = _field_table(what, codes, None, dev)
    fw, W, gap = _field_weights(what, field_weights, F, gap)
    return (ptr(codes), Vt, F, fw, gap), W, "_w"


def field_distances(Xq, Lq, Xr, Lr, codes, gap=None, out=None, field_weights=None):
    """The phonology-weighted edit distance of every (query, reference) pair (``slnlp_field_distances``, csrc/field_knn.hip):
    substituting a frame costs the number of fields in which the two tokens' rows of ``codes`` (int32 [Vt, F] on the device)
    differ -- F for a token outside the table, 0 for the same token -- inserting or deleting one costs ``gap`` (1..F; None: F).
    Rows as ``edit_distances`` -> uint16 [nq, nr]; 65535 where either row's length lies outside 0..64 (or beyond its row).  ``out``:
    the matrix to fill.  One launch on the current stream of ``Xq``'s device; no host wait.  ``field_weights`` (None: the call
    above, unchanged): F integers in 0..16 with sum W in 1..16 -- field f counts ``field_weights[f]``, a token outside the table
    costs W, ``gap`` lies in 1..W (None: W) and distances are at most 64 W (``slnlp_field_distances_w``)."""
    what = "field_distances"

    def metric(dev):
        args, _, w = _field_metric(what, codes, gap, field_weights, dev)
        return getattr(load(), "slnlp_field_distances" + w), args
    return _knn_distances(what, torch.uint16, 1, Xq, Lq, Xr, Lr, out, metric)


def field_knn_rows(Xq, Lq, Xr, Lr, codes, k, *, gap=None, radius=0, exclude=None, buf=None, scratch=None, field_weights=None):
    """``edit_knn_rows`` under the phonology-weighted distance of ``field_distances`` (``slnlp_field_knn_rows``): the same selection
    into the same ``buf`` (``edit_knn_buffers(nq, k, device)``; None: a new one), distances in field units, ``radius`` in 0..64 F.
    ``scratch``: a uint8 tensor of at least 2 nq nr bytes, 2-byte aligned (None: a new one; it holds the uint16 [nq, nr] matrix
    afterwards).  Three queued launches on the current stream of ``Xq``'s device; no host wait.  Returns ``buf``.
    ``field_weights`` (None: the call above, unchanged): the weighted metric of ``field_distances(field_weights=...)`` --
    ``gap`` in 1..W, ``radius`` in 0..64 W, distances in units of W (``slnlp_field_knn_rows_w``)."""
    what = "field_knn_rows"
    k = _int_in(what, "k", k, 1, _lib.EDIT_MAX_K)

    def metric(dev):
        args, unit, w = _field_metric(what, codes, gap, field_weights, dev)
        return getattr(load(), "slnlp_field_knn_rows" + w), args, _int_in(what, "radius", radius, 0, _lib.EDIT_MAX_LEN * unit)
    return _knn_rows(what, 2, 1, Xq, Lq, Xr, Lr, k, exclude, buf, scratch, metric)


def field_knn_logp(buf, Lq, Lr, yr, prior, F, *, weights="distance", tau=1.0, normalize=True, lam=1.0, out=None):
    """``edit_knn_logp`` for the neighbours of ``field_knn_rows`` (``slnlp_field_knn_logp``): distances are in units of ``F`` fields
    (1..16), so w = exp(-d / (tau n)) with n = F max(Lq, Lr, 1) when ``normalize``, else F -- ``tau`` is in frames in both metrics,
    and at F = 1 the vote is ``edit_knn_logp``'s bit for bit.  Two queued launches on the current stream of ``buf``'s device; no host
    wait.  Returns ``out``."""
    return _knn_logp("field_knn_logp", "slnlp_field_knn_logp", buf, Lq, Lr, yr, prior, ("F", F, 1, _lib.FIELD_MAX_FIELDS), weights, tau,
                     normalize, lam, out)


DUP_WIDTHS = {torch.uint8: 1, torch.uint16: 2}             # the bytes of a distance: edit_distances | edit_long_ / field_distances


def dup_groups_buffers(N, device):
    """The state and the outputs of one near-duplicate grouping of ``N`` rows (csrc/dup_groups.hip) as slices of ONE int32
    allocation, so that ``dup_groups_download`` is one copy:

        head int64 [8] | group int32 [N] | degree int32 [N] | parent int32 [N]

    and the forest begun (``slnlp_dup_groups_begin``: parent[i] = i, degree 0, head 0) on the current stream of ``device``; no host
    wait.  ``parent`` is the device-resident forest the chunks are linked into; it is never downloaded."""
    _lib.require_gpu()
    N = _int_in("dup_groups_buffers", "N", N, 1, _lib.EDIT_MAX_ROWS)
    device = torch.device(device)
    with torch.cuda.device(device):
        p = _packed.Packed(torch.int32, (("head", torch.int64, _lib.DUP_HEAD_BYTES // 8, 8), ("group", torch.int32, N, 4),
                                         ("degree", torch.int32, N, 4), ("parent", torch.int32, N, 4)), device)
        buf = _packed_dict(p, (N,))
        check(load().slnlp_dup_groups_begin(ptr(buf["parent"]), ptr(buf["degree"]), N, ptr(buf["head"]), stream_ptr()), "dup_groups_buffers")
    return buf


def dup_groups_link(dist, q0, radius, buf):
    """Link one chunk of distances into ``buf``'s forest (``slnlp_dup_groups_link``): ``dist`` a contiguous uint8 or uint16 [nq, N]
    device tensor, what ``edit_distances`` / ``edit_long_distances`` / ``field_distances`` write for the data set's rows ``q0 .. q0 +
    nq - 1`` against all N of them; ``radius`` in 0..254 (uint8) or 0..65534 (uint16).  Every row of the data set is linked exactly
    once.  One launch on the current stream of ``dist``'s device; no host wait.  Returns ``buf``."""
    what = "dup_groups_link"
    _packed_buf(what, buf, "dup_groups_buffers(N, device)", (), None, more=1)
    N, = buf["shape"]
    dev = buf["flat"].device
    if not (torch.is_tensor(dist) and dist.dtype in DUP_WIDTHS and dist.dim() == 2 and dist.shape[1] == N and dist.shape[0] >= 1
            and dist.is_contiguous() and dist.device == dev):
        raise ValueError(f"{what}: dist must be a contiguous uint8 or uint16 [nq >= 1, {N}] tensor on {dev}")
    width, nq = DUP_WIDTHS[dist.dtype], int(dist.shape[0])
    q0 = _int_in(what, "q0", q0, 0, N - 1)
    radius = _int_in(what, "radius", radius, 0, 254 if width == 1 else 65534)
    _lib.require_gpu()
    with torch.cuda.device(dev):
        check(load().slnlp_dup_groups_link(ptr(dist), width, nq, N, q0, radius, ptr(buf["parent"]), ptr(buf["degree"]), ptr(buf["head"]),
                                           stream_ptr()), what)
    return buf


def dup_groups_finish(buf):
    """Resolve ``buf``'s forest (``slnlp_dup_groups_finish``): ``buf["group"]`` = every row's root, the lowest row index of its
    component; the head gets the groups and the edges.  Two launches on the current stream of ``buf``'s device; no host wait.
    Returns ``buf``."""
    what = "dup_groups_finish"
    _packed_buf(what, buf, "dup_groups_buffers(N, device)", (), None, more=1)
    N, = buf["shape"]
    _lib.require_gpu()
    with torch.cuda.device(buf["flat"].device):
        check(load().slnlp_dup_groups_finish(ptr(buf["parent"]), N, ptr(buf["group"]), ptr(buf["head"]), stream_ptr()), what)
    return buf


def dup_groups_download(buf):
    """What a grouping hands to the host in ONE device-to-host copy: {head int64 [8] = (groups, edges within the radius, unusable
    rows, code, the degree sum, 0, 0, 0), group int32 [N], degree int32 [N]}.  A code other than 0 -- a kernel loop ran out of its N +
    1 rounds, which the forest's invariants rule out -- raises RuntimeError."""
    _packed_buf("dup_groups_download", buf, "dup_groups_buffers(N, device)", (), None, more=1)
    out = buf["packed"].cut("head", "degree")
    if int(out["head"][3]) != 0:
        raise RuntimeError(f"dup_groups_download: the device reports code {int(out['head'][3])}: a union-find loop exhausted its bound of N + 1 "
                           "rounds; the groups are not to be used")
    return out


GLOSS_MAKER = "gloss_structure_buffers(N, C, labels, max_distance, device)"


def gloss_structure_buffers(N, C, labels, max_distance, device):
    """The state and the outputs of one gloss-structure pass over ``N`` rows of ``C`` classes (csrc/gloss_structure.hip) as slices
    of ONE int64 allocation, so that ``gloss_structure_download`` is one copy:

        head int64 [8] | own uint32 [N] | other uint32 [N] | other_class int32 [N] | count int32 [C] | medoid int32 [C]
                       | class_sum int64 [C, C] | med_sum int64 [C]

    (``own`` and ``other`` are held as int32 tensors: the same bits).  ``labels``: N integers in -1..C-1 (-1: the row is left
    out), a host array or a tensor; they are uploaded as int32 (``buf["label"]``) and the pass begun
    (``slnlp_gloss_structure_begin``: the class counts taken, the sums zeroed) on the current stream of ``device``; no host wait.
    ``max_distance``: the metric's bound -- 64, ``max_len``, 64 F or 64 W; ``max_distance * N`` must stay below 2^32.  A label
    outside -1..C-1 is found on the device and raised by ``gloss_structure_download``."""
    what = "gloss_structure_buffers"
    _lib.require_gpu()
    N = _int_in(what, "N", N, 1, _lib.EDIT_MAX_ROWS)
    C = _int_in(what, "C", C, 1, _lib.GLOSS_MAX_CLASSES)
    max_distance = _int_in(what, "max_distance", max_distance, 1, 65534)
    if max_distance * N >= 2 ** 32:
        raise ValueError(f"{what}: max_distance={max_distance} times N={N} reaches 2^32: a row's sum over one class must fit 32 bits")
    device = torch.device(device)
    lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels))
    if lab.dim() != 1 or lab.shape[0] != N or lab.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: labels must be {N} int32 or int64 values in -1..{C - 1}")
    with torch.cuda.device(device):
        label = lab.to(device=device, dtype=torch.int32).contiguous()
        p = _packed.Packed(torch.int64, (("head", torch.int64, _lib.GLOSS_HEAD_BYTES // 8, 8), ("own", torch.int32, N, 4),
                                         ("other", torch.int32, N, 4), ("other_class", torch.int32, N, 4), ("count", torch.int32, C, 4),
                                         ("medoid", torch.int32, C, 4), ("class_sum", torch.int64, (C, C), 8), ("med_sum", torch.int64, C, 8)),
                           device)
        buf = _packed_dict(p, (N, C), label=label, max_distance=max_distance)
        check(load().slnlp_gloss_structure_begin(ptr(label), N, C, max_distance, ptr(buf["count"]), ptr(buf["class_sum"]), ptr(buf["med_sum"]),
                                                 ptr(buf["medoid"]), ptr(buf["head"]), stream_ptr()), what)
    return buf


def _gloss_buf(what, buf):
    _packed_buf(what, buf, GLOSS_MAKER, (), None, more=2)
    if "label" not in buf or "class_sum" not in buf:
        raise ValueError(f"{what}: buf must be {GLOSS_MAKER}")
    return buf["shape"]


def gloss_structure_rows(dist, q0, buf):
    """One chunk of distances into ``buf``'s sums (``slnlp_gloss_structure_rows``): ``dist`` a contiguous uint8 or uint16 [nq, N]
    device tensor, what ``edit_distances`` / ``edit_long_distances`` / ``field_distances`` write for the data set's rows ``q0 .. q0
    + nq - 1`` against all N of them.  Every row of the data set arrives exactly once, in any order.  One launch on the current
    stream of ``dist``'s device; no host wait.  Returns ``buf``."""
    what = "gloss_structure_rows"
    N, C = _gloss_buf(what, buf)
    dev = buf["flat"].device
    if not (torch.is_tensor(dist) and dist.dtype in DUP_WIDTHS and dist.dim() == 2 and dist.shape[1] == N and dist.shape[0] >= 1
            and dist.is_contiguous() and dist.device == dev):
        raise ValueError(f"{what}: dist must be a contiguous uint8 or uint16 [nq >= 1, {N}] tensor on {dev}")
    width, nq = DUP_WIDTHS[dist.dtype], int(dist.shape[0])
    q0 = _int_in(what, "q0", q0, 0, N - 1)
    _lib.require_gpu()
    with torch.cuda.device(dev):
        check(load().slnlp_gloss_structure_rows(ptr(dist), width, nq, N, q0, ptr(buf["label"]), C, ptr(buf["count"]), ptr(buf["own"]),
                                                ptr(buf["other"]), ptr(buf["other_class"]), ptr(buf["class_sum"]), ptr(buf["med_sum"]),
                                                ptr(buf["head"]), stream_ptr()), what)
    return buf


def gloss_structure_finish(buf):
    """The medoids of ``buf``'s classes and the head's class count (``slnlp_gloss_structure_finish``).  Two launches on the current
    stream of ``buf``'s device; no host wait.  Returns ``buf``."""
    what = "gloss_structure_finish"
    N, C = _gloss_buf(what, buf)
    _lib.require_gpu()
    with torch.cuda.device(buf["flat"].device):
        check(load().slnlp_gloss_structure_finish(ptr(buf["label"]), ptr(buf["own"]), ptr(buf["med_sum"]), N, C, ptr(buf["medoid"]),
                                                  ptr(buf["head"]), stream_ptr()), what)
    return buf


def gloss_structure_download(buf):
    """What a gloss-structure pass hands to the host in ONE device-to-host copy: {head int64 [8] = (labelled rows, non-empty
    classes, rows left out, code, the sum of own, 0, 0, 0), own uint32 [N], other uint32 [N], other_class int32 [N], count int32
    [C], medoid int32 [C], class_sum int64 [C, C]}.  A code other than 0 raises RuntimeError: bit 0 -- the sentinel of an
    unusable row met at a pair of two LABELLED rows (the caller labels such rows -1); bit 1 -- a label outside -1..C-1."""
    what = "gloss_structure_download"
    _gloss_buf(what, buf)
    out = buf["packed"].cut("head", "class_sum")
    code = int(out["head"][3])
    if code != 0:
        why = [w for bit, w in ((1, "a distance sentinel at a pair of labelled rows (a row the metric refuses must be labelled -1)"),
                                (2, f"a label outside -1..{buf['shape'][1] - 1}")) if code & bit]
        raise RuntimeError(f"{what}: the device reports code {code}: {'; '.join(why)}; the result is not to be used")
    out["own"], out["other"] = out["own"].view(np.uint32), out["other"].view(np.uint32)
    return out


def loo_objective_table(slots, device):
    """The table ``loo_objective`` fills: an int64 [slots, 4] device tensor of zeros, one 32-byte slot a candidate"""
    slots = _int_in("loo_objective_table", "slots", slots, 1, _lib.LOO_MAX_SLOTS)
    return torch.zeros(slots, _lib.LOO_SLOT_BYTES // 8, dtype=torch.int64, device=device)


def loo_objective(logp, y, table, slot):
    """What a search over candidate metrics ranks by (``slnlp_loo_objective``, csrc/score.hip): of the float32 log-probs ``logp``
    [N, V] and the labels ``y`` int64 [N], into slot ``slot`` of ``table`` (``loo_objective_table``) the number of rows whose
    arg-max -- the lowest index on a tie -- is the label, the fp64 sum of -logp[i, y_i] in a fixed order that depends on N alone,
    the rows that hold a NaN and the rows whose label lies outside the classes (both count as wrong and add nothing).  One launch
    on the current stream of ``logp``'s device; no host wait.  Returns ``table``."""
    what = "loo_objective"
    N, V, ld = _logp_matrix(what, logp)
    _labels(what, y, logp.device, N)
    if not (torch.is_tensor(table) and table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == _lib.LOO_SLOT_BYTES // 8
            and 1 <= table.shape[0] <= _lib.LOO_MAX_SLOTS and table.is_contiguous() and table.device == logp.device):
        raise ValueError(f"{what}: table must be loo_objective_table(slots, device) on {logp.device}: a contiguous int64 [slots, 4] tensor")
    C = int(table.shape[0])
    slot = _int_in(what, "slot", slot, 0, C - 1)
    _lib.require_gpu()
    with torch.cuda.device(logp.device):
        check(load().slnlp_loo_objective(ptr(logp), ld, ptr(y), N, V, ptr(table), C, slot, stream_ptr()), what)
    return table


def loo_objective_download(table):
    """``loo_objective``'s table on the host in ONE device-to-host copy: {right int64 [C], sum float64 [C], nan_rows int64 [C],
    bad_labels int64 [C]}"""
    t = table.cpu()
    return {"right": t[:, 0].numpy().copy(), "sum": t[:, 1].contiguous().view(torch.float64).numpy().copy(), "nan_rows": t[:, 2].numpy().copy(),
            "bad_labels": t[:, 3].numpy().copy()}


def scatter_logp(logp, rows, out, state=None):
    """``out[rows[i], :] = `` row i of ``logp`` float32 [n, V] (``slnlp_scatter_logp``): with ``state`` (a calibration state whose beta
    is read on the device) the row ``scale_logp`` would write, bit for bit; with None the float32 values themselves.  ``rows``: a
    contiguous int64 [n] device tensor of DISTINCT indices (the caller checks: this is how ``OutOfFold`` assembles its folds, which
    it has validated as a partition); an index outside ``out``'s rows is skipped on the device.  ``out``: a float32 [N_out, V]
    device tensor that does not overlap ``logp``; rows no index names keep what they held.  Runs on the current stream of
    ``logp``'s device; no host wait.  Returns ``out``."""
    _lib.require_gpu()
    what = "scatter_logp"
    n, V, ld = _logp_matrix(what, logp)
    _tensor(what, "rows", rows, logp.device, torch.int64, n)
    if state is not None:
        _cal_state(what, state, logp.device)
    if not (torch.is_tensor(out) and out.device == logp.device and out.dim() == 2 and out.shape[1] == V and out.shape[0] >= 1):
        raise ValueError(f"{what}: out must be a float32 [N_out, {V}] tensor on {logp.device}")
    N_out, _, ld_out = _logp_matrix(what + " (out)", out)
    with torch.cuda.device(logp.device):
        check(load().slnlp_scatter_logp(ptr(logp), ld, n, V, ptr(state), ptr(rows), ptr(out), ld_out, N_out, stream_ptr()), what)
    return out


def bootstrap_buffers(B, V, Q, counts, device):
    """The output tensors of ``bootstrap_scores`` for ``B`` replicates over ``V`` classes with ``Q`` value columns -- stats
    float64 [B, 9 + Q] and, with ``counts``, counts int32 [B, 3 V + 1] (else None) -- as slices of ONE allocation, so
    ``bootstrap_download`` is one copy."""
    p = _packed.Packed(torch.float64, (("stats", torch.float64, (B, _lib.BOOT_FIXED + Q), 8),)
                       + ((("counts", torch.int32, (B, 3 * V + 1), 4),) if counts else ()), device)
    return p.view("stats"), (p.view("counts") if counts else None)


def bootstrap_download(out):
    """``bootstrap_scores``' result as numpy arrays ``(stats float64 [B, 9 + Q], counts int32 [B, 3 V + 1] or None)``: one
    device-to-host copy when they are ``bootstrap_buffers``' slices of one allocation (it waits for the launch), two otherwise."""
    if out[1] is None:
        return out[0].cpu().numpy(), None
    return _packed.download(out, torch.float64)


def bootstrap_scores(y, pred, rank, values=None, *, n_classes, top_k=0, replicates, seed, counts=False, out=None):
    """``replicates`` bootstrap replicates of the scoring metrics of one set of predictions (``slnlp_bootstrap_scores``,
    include/slnlp.h): the labels ``y`` int64 [N], ``score_rows``' ``pred`` and ``rank`` int32 [N] (``rank`` may be None when
    ``top_k`` is 0) and ``values`` float64 [N, Q] with unit column stride, Q <= 8 (rows may be padded: ``stride(0) >= Q`` --
    ``reliability_rows``' ``rows[:, :3]`` directly: conf, brier, nll; None: Q = 0) are resampled with replacement, every replicate
    from N draws that depend on ``(seed, replicate, N)`` alone -- two calls with one seed resample two fits alike.  Returns
    ``(stats float64 [replicates, 9 + Q], counts)``, device tensors sliced from one allocation: the columns of ``stats`` are
    ``metrics.BOOT_COLUMNS`` (``top_k_accuracy`` is NaN with ``top_k=0``, else top-``top_k`` accuracy, k in [1, n_classes)), then
    the means of the value columns; ``counts`` is int32 [replicates, 3 V + 1] (``score_rows``' layout per replicate) with
    ``counts=True``, else None.  ``out``: such a pair to fill.  Runs on the current stream of ``y``'s device; no host wait."""
    _lib.require_gpu()
    what = "bootstrap_scores"
    if not (y.is_cuda and y.dtype == torch.int64 and y.dim() == 1 and y.numel() >= 1 and y.is_contiguous()):
        raise ValueError(f"{what}: y must be a contiguous int64 [N] device tensor, got {y.dtype} {tuple(y.shape)} on {y.device}")
    N = y.numel()
    V = _int_in(what, "n_classes", n_classes, 1, _lib.CONFUSION_MAX_V)
    B = _int_in(what, "replicates", replicates, 1, _lib.BOOT_MAX_REPLICATES)
    seed = _int_in(what, "seed", seed, 0, 2 ** 64 - 1)
    top_k = _int_in(what, "top_k", top_k, 0, max(V - 1, 0))
    for name, t in (("pred", pred), ("rank", rank)):
        if t is None and name == "rank" and top_k == 0:
            continue
        if t is None:
            raise ValueError(f"{what}: {name} must be a contiguous int32 [{N}] tensor on {y.device}")
        _tensor(what, name, t, y.device, torch.int32, N)
    Q, ldv = 0, 0
    if values is not None:
        if not (values.device == y.device and values.dtype == torch.float64 and values.dim() == 2 and values.shape[0] == N
                and 1 <= values.shape[1] <= _lib.BOOT_MAX_VALUES and (values.stride(1) == 1 or values.shape[1] == 1)
                and (N == 1 or values.stride(0) >= values.shape[1])):
            raise ValueError(f"{what}: values must be a float64 [{N}, 1..{_lib.BOOT_MAX_VALUES}] tensor on {y.device} with unit column "
                             f"stride, got {values.dtype} {tuple(values.shape)} strides {values.stride()} on {values.device}")
        Q = int(values.shape[1])
        ldv = int(values.stride(0)) if N > 1 else max(Q, int(values.stride(0)))
    with torch.cuda.device(y.device):
        if out is None:
            out = bootstrap_buffers(B, V, Q, bool(counts), y.device)
        stats, cnt = out
        must_be = f"(float64 [{B}, {_lib.BOOT_FIXED + Q}], int32 [{B}, {3 * V + 1}] or None) on {y.device}"
        _tensor(what, "out", stats, y.device, torch.float64, (B, _lib.BOOT_FIXED + Q), must_be)
        if cnt is not None:
            _tensor(what, "out", cnt, y.device, torch.int32, (B, 3 * V + 1), must_be)
        check(load().slnlp_bootstrap_scores(ptr(y), ptr(pred), ptr(rank) if top_k else None, ptr(values), ldv, Q, N, V, top_k, B, seed,
                                            ptr(stats), ptr(cnt), stream_ptr()), what)
    return out


def score_interval_buffers(N, V, B, device, bins=15):
    """Every device buffer of one bootstrap of an [N, V] set of log-probs (``NeuralNetClassifier.score_interval``) as slices of ONE
    float64 allocation, what the host reads first:

        stats [B, 9 + 3] | table [bins + 1, 4] | pred [N] | picked float32 [N] | rank [N] | counts [3 V + 1] | rows [N, 4]

    (pad entries keep table and rows 32-byte aligned).  ``score`` = (pred, picked, rank, counts) is ``score_rows``' ``out``,
    ``reliability`` = (rows, table) ``reliability_rows``', ``boot`` = (stats, None) ``bootstrap_scores``'; the per-row terms never
    leave the device (``score_interval_download``)."""
    what = "score_interval_buffers"
    N, V = _int_in(what, "N", N, 1, 2 ** 31 - 1), _int_in(what, "V", V, 1, _lib.CONFUSION_MAX_V)
    B, bins = _int_in(what, "B", B, 1, _lib.BOOT_MAX_REPLICATES), _int_in(what, "bins", bins, 1, _lib.REL_MAX_BINS)
    p = _packed.Packed(torch.float64, (("stats", torch.float64, (B, _lib.BOOT_FIXED + 3), 8), ("table", torch.float64, (bins + 1, 4), 32),
                                       *_score_pieces(N, V), ("rows", torch.float64, (N, 4), 32)), device)
    return {"flat": p.flat, "shape": (N, V, B, bins), "head": p.end("counts"), "at": (p.begin("table"), p.begin("pred")), "packed": p,
            "score": p.views("pred", "picked", "rank", "counts"), "reliability": p.views("rows", "table"), "boot": (p.view("stats"), None)}


def score_interval_rows(logp, y, buf, *, top_k=0, seed=0, state=None):
    """One bootstrap on the device, into ``score_interval_buffers``' slices: ``score_rows``, ``reliability_rows`` (at ``state``'s
    beta; None: 1) and ``bootstrap_scores`` on what the two left -- pred, rank and the (conf, brier, nll) columns.  Runs on the
    current stream of ``logp``'s device; no host wait.  Returns ``buf``."""
    N, V, B, bins = buf["shape"]
    pred, _, rank, _ = score_rows(logp, y, out=buf["score"])
    rows, _ = reliability_rows(logp, y, bins=bins, state=state, out=buf["reliability"])
    bootstrap_scores(y, pred, rank, rows[:, :3], n_classes=V, top_k=top_k, replicates=B, seed=seed, out=buf["boot"])
    return buf


def score_interval_download(buf):
    """What ``score_interval_rows`` hands to the host, in ONE device-to-host copy (it waits for the launches): a dict of numpy
    arrays -- ``stats`` float64 [B, 12], ``table`` float64 [bins + 1, 4], ``pred`` int32 [N], ``rank`` int32 [N], ``counts`` int64
    [3 V + 1]."""
    import numpy as np
    h = buf["packed"].cut("stats", "counts")
    return {"stats": h["stats"], "table": h["table"], "pred": h["pred"], "rank": h["rank"], "counts": h["counts"].astype(np.int64)}


def ensemble_rows(logps, states=None, weights=None, voting="soft", diagnostics=True, out=None):
    """K fits' log-probs combined on the device (``slnlp_ensemble_rows``, include/slnlp.h): ``logps`` is a list of 1..32 float32
    [N, V] device tensors (rows may be padded: ``stride(0) >= V``), ``states`` a list of calibration states (``fit_temperature`` /
    ``temperature_state``) or Nones -- member k enters as softmax(beta_k logp_k), beta_k read on the device, None: 1 --
    ``weights`` K finite numbers > 0 (normalised by the call) or None: equal; ``voting`` "soft", the mean of the probabilities, or
    "log", their weighted geometric mean renormalised.  Returns ``(out float32 [N, V], rows float64 [N, 4] or None)``: the
    combined log-probs, in the layout every row op here reads, and per row (total entropy, expected member entropy, mutual
    information, number of members whose arg-max is not the ensemble's) -- (NaN, NaN, NaN, -2) and a NaN ``out`` row where a
    member's row holds a NaN.  ``diagnostics=False`` forms no rows.  ``out``: a float32 [N, V] tensor to fill, no member's memory.
    Runs on the current stream of the members' device; no host wait."""
    _lib.require_gpu()
    what = "ensemble_rows"
    logps = list(logps) if isinstance(logps, (list, tuple)) else []
    K = len(logps)
    if not 1 <= K <= _lib.ENSEMBLE_MAX_MEMBERS:
        raise ValueError(f"{what}: logps must be a list of 1..{_lib.ENSEMBLE_MAX_MEMBERS} tensors")
    if voting not in _lib.VOTING:
        raise ValueError(f"{what}: voting={voting!r}, expected one of {tuple(_lib.VOTING)}")
    N, V, _ = _logp_matrix(what, logps[0])
    dev = logps[0].device
    lds = []
    for k, z in enumerate(logps):
        n, v, ld = _logp_matrix(f"{what} (member {k})", z)
        if (n, v) != (N, V) or z.device != dev:
            raise ValueError(f"{what}: member {k} is {tuple(z.shape)} on {z.device}, member 0 is {(N, V)} on {dev}")
        lds.append(ld)
    states = [None] * K if states is None else list(states)
    if len(states) != K:
        raise ValueError(f"{what}: {len(states)} states for {K} members")
    for st in states:
        if st is not None:
            _cal_state(what, st, dev)
    if weights is not None:
        weights = [float(w) for w in weights]
        if len(weights) != K or not all(0.0 < w < float("inf") for w in weights):
            raise ValueError(f"{what}: weights={weights!r}, expected {K} finite numbers above 0")
    with torch.cuda.device(dev):
        out, ld_out = _out_like(what, logps[0], out)
        rows = torch.empty(N, 4, dtype=torch.float64, device=dev) if diagnostics else None
        check(load().slnlp_ensemble_rows((C.c_void_p * K)(*[ptr(z) for z in logps]), (C.c_int64 * K)(*lds),
                                         (C.c_void_p * K)(*[ptr(st) for st in states]),
                                         (C.c_double * K)(*weights) if weights is not None else None, K, N, V, _lib.VOTING[voting],
                                         ptr(out), ld_out, ptr(rows), stream_ptr()), what)
    return out, rows


def ensemble_download(res, per_row=False):
    """``ensemble_rows``' diagnostics as ``metrics.uncertainty_summary``'s dict; ``per_row=True`` adds ``per_row``, the float64
    [N, 4] rows.  ONE device-to-host copy, of the rows (it waits for the launch); the combined log-probs stay on the device."""
    from . import metrics
    if res[1] is None:
        raise ValueError("ensemble_download: the call formed no diagnostics (diagnostics=False)")
    rows = res[1].cpu().numpy()
    got = metrics.uncertainty_summary(rows)
    if per_row:
        got["per_row"] = rows
    return got


class ParamGroupTable:
    """Device copy of a per-parameter-group segment table over an arena of ``n`` floats (``slnlp_param_groups_create``):
    segment s covers floats [seg_begin[s], seg_begin[s + 1]) -- the last one to ``n`` -- in group seg_group[s]; group g decays
    with weight_decay[g].  The groups' learning rates are a device tensor given to each step."""

    def __init__(self, n, seg_begin, seg_group, weight_decay):
        import ctypes as C
        _lib.require_gpu()
        self.n, self.n_groups, self.handle = int(n), len(weight_decay), C.c_void_p()
        check(load().slnlp_param_groups_create(self.n, len(seg_begin), (C.c_int64 * len(seg_begin))(*seg_begin),
                                               (C.c_int32 * len(seg_group))(*seg_group), len(weight_decay),
                                               (C.c_float * len(weight_decay))(*weight_decay), stream_ptr(), C.byref(self.handle)),
              "param_groups_create")

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                load().slnlp_param_groups_destroy(h)
            except Exception:                            # interpreter shutdown: the module globals are already gone
                pass
            self.handle = None


def clip_sgd_step_groups(params, grads, buf, table, lr_dev, step_count, *, momentum=0.9, dampening=0.0, nesterov=False, max_norm=0.5,
                         skip=(0, 0)):
    """``clip_sgd_step_ex`` with lr (``lr_dev`` [groups], device) and weight decay per parameter group (``table``: a
    ``ParamGroupTable``).  Returns the pre-clip norm [1]."""
    _lib.require_gpu()
    partials = torch.empty(1024, dtype=torch.float32, device=params.device)
    norm = torch.empty(1, dtype=torch.float32, device=params.device)
    assert lr_dev.numel() == table.n_groups
    check(load().slnlp_clip_sgd_step_groups(ptr(params), ptr(grads), ptr(buf), params.numel(), table.handle, ptr(lr_dev), momentum,
                                            dampening, int(bool(nesterov)), max_norm, ptr(partials), ptr(norm), ptr(step_count),
                                            skip[0], skip[1], stream_ptr()), "clip_sgd_step_groups")
    return norm


def clip_adam_step_groups(params, grads, exp_avg, exp_avg_sq, table, lr_dev, step_count, *, betas=(0.9, 0.999), eps=1e-8,
                          decoupled=False, max_norm=0.5, skip=(0, 0)):
    """``clip_adam_step`` (``decoupled``: ``clip_adamw_step``) with lr and weight decay per parameter group, as
    ``clip_sgd_step_groups``.  Returns the pre-clip norm [1]."""
    _lib.require_gpu()
    partials = torch.empty(1024, dtype=torch.float32, device=params.device)
    norm = torch.empty(1, dtype=torch.float32, device=params.device)
    assert lr_dev.numel() == table.n_groups
    check(load().slnlp_clip_adam_step_groups(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), table.handle,
                                             ptr(lr_dev), betas[0], betas[1], eps, int(bool(decoupled)), max_norm, ptr(partials),
                                             ptr(norm), ptr(step_count), skip[0], skip[1], stream_ptr()), "clip_adam_step_groups")
    return norm


def dropout_mask(R, C_, p, site, rng):
    _lib.require_gpu()
    out = torch.empty(R, C_, dtype=torch.float32, device=rng.device)
    check(load().slnlp_dropout_mask(ptr(out), R, C_, p, site, ptr(rng), stream_ptr()), "dropout_mask")
    return out


def dir_struct(cls, **fields):
    """One direction's argument struct of the recurrent entry points (``_lib.RnnCellDir``, ``RnnStepDir``, ``RnnLayerDir``,
    ``RnnCellBwdDir``): tensors (views included) become their device pointers, None a null pointer, numbers stay."""
    return cls(**{k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in fields.items()})


def _dirs(cls, dirs):
    assert len(dirs) in (1, 2) and all(isinstance(d, cls) for d in dirs)
    return (cls * len(dirs))(*dirs)


def rnn_cell_fwd(lstm, dirs, *, B, Hd, lengths=None, fill=0.0, ld_out=0, drop_p=0.0, drop_site=0, rng=None):
    """One timestep of the point-wise cell for 1 or 2 directions (``dirs``: ``_lib.RnnCellDir``), in place on their buffers."""
    _lib.require_gpu()
    check(load().slnlp_rnn_cell_fwd(int(lstm), _dirs(_lib.RnnCellDir, dirs), len(dirs), B, Hd, ptr(lengths), fill, ld_out, drop_p,
                                    drop_site, ptr(rng), stream_ptr()), "rnn_cell_fwd")


def rnn_cell_bwd(lstm, dirs, *, B, Hd, lengths=None, ld_dout=0, drop_p=0.0, drop_site=0, rng=None):
    """Backward of one timestep of the cell (``dirs``: ``_lib.RnnCellBwdDir``): writes dgx, dgh, carry, updates dc_state."""
    _lib.require_gpu()
    check(load().slnlp_rnn_cell_bwd(int(lstm), _dirs(_lib.RnnCellBwdDir, dirs), len(dirs), B, Hd, ptr(lengths), ld_dout, drop_p,
                                    drop_site, ptr(rng), stream_ptr()), "rnn_cell_bwd")


def rnn_step_fwd(lstm, dirs, *, B, Hd, lengths=None, fill=0.0, ld_out=0, drop_p=0.0, drop_site=0, rng=None, precision=3):
    """Recurrent product + cell of one timestep in one launch (``dirs``: ``_lib.RnnStepDir``)."""
    _lib.require_gpu()
    check(load().slnlp_rnn_step_fwd(int(lstm), _dirs(_lib.RnnStepDir, dirs), len(dirs), B, Hd, ptr(lengths), fill, ld_out, drop_p,
                                    drop_site, ptr(rng), precision, stream_ptr()), "rnn_step_fwd")


def rnn_step_bwd(lstm, dirs, *, B, Hd, lengths=None, ld_dout=0, drop_p=0.0, drop_site=0, rng=None, precision=3):
    """Recurrent data gradient of the step before + this step's cell backward in one launch (``dirs``: ``_lib.RnnStepBwdDir``)."""
    _lib.require_gpu()
    check(load().slnlp_rnn_step_bwd(int(lstm), _dirs(_lib.RnnStepBwdDir, dirs), len(dirs), B, Hd, ptr(lengths), ld_dout, drop_p,
                                    drop_site, ptr(rng), precision, stream_ptr()), "rnn_step_bwd")


def bahdanau_fwd(q, proj_key, value, w_energy, ids, pad_idx, *, B, S, Hd):
    """-> (alphas [B, S], ctx [B, 2 Hd]); proj_key [S*B, Hd] / value [S*B, 2 Hd] rows time-major, ids int64 [B, S]."""
    _lib.require_gpu()
    alphas = torch.empty(B, S, dtype=torch.float32, device=q.device)
    ctx = torch.empty(B, 2 * Hd, dtype=torch.float32, device=q.device)
    check(load().slnlp_bahdanau_fwd(ptr(q), ptr(proj_key), ptr(value), ptr(w_energy), ptr(ids), ids.stride(0), pad_idx, B, S, Hd,
                                    ptr(alphas), ptr(ctx), stream_ptr()), "bahdanau_fwd")
    return alphas, ctx


def bahdanau_bwd(q, proj_key, value, w_energy, alphas, dctx, *, B, S, Hd):
    """-> (dq [B, Hd], dproj_key [S*B, Hd], dvalue [S*B, 2 Hd], dw_energy [Hd])"""
    _lib.require_gpu()
    dq = torch.empty_like(q)
    dpk = torch.empty_like(proj_key)
    dval = torch.empty_like(value)
    part = torch.empty(B, Hd, dtype=torch.float32, device=q.device)
    dwe = torch.empty(Hd, dtype=torch.float32, device=q.device)
    check(load().slnlp_bahdanau_bwd(ptr(q), ptr(proj_key), ptr(value), ptr(w_energy), ptr(alphas), ptr(dctx), B, S, Hd, ptr(dq),
                                    ptr(dpk), ptr(dval), ptr(part), ptr(dwe), stream_ptr()), "bahdanau_bwd")
    return dq, dpk, dval, dwe


def gather_batch(X, lengths, y, order, row0, B, out=None):
    """One batch in visit order: rows ``order[row0 : row0 + B]`` of the device-resident dataset ``X`` int64 [rows, S] /
    ``lengths`` int64 [rows] or None / ``y`` int64 [rows]; ``order`` None: rows ``row0 : row0 + B``.  ``out``: staging buffers
    ``(X_out [>= B, S], len_out [>= B] or None, y_out [>= B])`` to fill (a captured graph's, a fit's); None allocates them.
    Returns the filled ``(X_out[:B], len_out[:B] or None, y_out[:B])``.  The order's indices are the caller's contract
    (``slnlp.sampler.check_order`` checks a host order before it is uploaded)."""
    _lib.require_gpu()
    rows, S = X.shape
    row0, B = int(row0), int(B)
    limit = rows if order is None else int(order.numel())
    if B < 1 or row0 < 0 or row0 + B > limit:
        raise ValueError(f"gather_batch: rows [{row0}, {row0 + B}) outside 0..{limit}")
    if out is None:
        out = (torch.empty(B, S, dtype=torch.int64, device=X.device),
               None if lengths is None else torch.empty(B, dtype=torch.int64, device=X.device),
               torch.empty(B, dtype=torch.int64, device=X.device))
    Xo, Lo, yo = out
    if lengths is None:
        Lo = None
    for t in (X, lengths, y, order, Xo, Lo, yo):
        assert t is None or (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()), "gather_batch: contiguous int64 device tensors"
    assert Xo.shape[0] >= B and Xo.shape[1] == S and yo.shape[0] >= B and (Lo is None or Lo.shape[0] >= B) and y.shape[0] == rows
    check(load().slnlp_gather_batch(ptr(X), ptr(lengths), ptr(y), ptr(order), row0, B, S, ptr(Xo), ptr(Lo), ptr(yo), stream_ptr()),
          "gather_batch")
    return Xo[:B], (None if Lo is None else Lo[:B]), yo[:B]


def augment_rows(X, L, pad, unk, p_drop, p_mask, seed, epoch, out=None):
    """One epoch's augmented copy of the device-resident rows ``X`` int64 [n, S] / ``L`` int64 [n] (``slnlp_augment_rows``,
    csrc/augment.hip): every position below a row's length is dropped with probability ``p_drop`` (the rest closes up; a row
    never loses all of its positions) and, when kept, replaced by ``unk`` with probability ``p_mask``; the tail is ``pad``.  A
    function of (X, L, seed, epoch) alone, drawn on the current stream: one launch, no host synchronisation.  ``out``: the
    pair ``(X_out [n, S], L_out [n])`` to fill -- never ``X`` / ``L`` themselves; None allocates it.  Returns the pair."""
    _lib.require_gpu()
    n, S = X.shape
    if out is None:
        out = (torch.empty_like(X), torch.empty_like(L))
    Xo, Lo = out
    for t in (X, L, Xo, Lo):
        assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous(), "augment_rows: contiguous int64 device tensors"
    assert L.shape == (n,) and Xo.shape == (n, S) and Lo.shape == (n,), "augment_rows: X [n, S], L [n] and outputs of the same shapes"
    check(load().slnlp_augment_rows(ptr(X), ptr(L), n, S, int(pad), int(unk), float(p_drop), float(p_mask), int(seed) % (1 << 64),
                                    int(epoch), ptr(Xo), ptr(Lo), stream_ptr()), "augment_rows")
    return Xo, Lo


class BalancePlan:
    """The per-class tables of a class-balanced epoch draw over the labels ``y`` (host int64 [n], values in
    ``[0, n_classes)``), in device memory the handle owns (``slnlp_balance_plan_create``).  ``rows``: the ``n_bal`` rows every
    epoch visits.  ``order(y_dev, seed, epoch)`` draws one epoch's visit order on the current stream: two launches, no host
    synchronisation, no upload.  A plan serves one draw at a time (include/slnlp.h)."""

    def __init__(self, y, n_classes):
        import ctypes as C
        import numpy as np
        _lib.require_gpu()
        y = np.ascontiguousarray(y, dtype=np.int64)
        if y.ndim != 1:
            raise ValueError(f"BalancePlan: labels of shape {y.shape}, expected one dimension")
        self.n, self.handle = int(y.size), C.c_void_p()
        check(load().slnlp_balance_plan_create(y.ctypes.data, self.n, int(n_classes), stream_ptr(), C.byref(self.handle)),
              "balance_plan_create")
        self.rows = int(load().slnlp_balance_plan_rows(self.handle))

    def order(self, y_dev, seed, epoch, out=None, want_labels=True):
        """-> (order int64 [rows], labels in visit order int64 [rows] or None), device tensors; ``out``: the pair to fill."""
        dev = y_dev.device
        assert y_dev.is_cuda and y_dev.dtype == torch.int64 and y_dev.is_contiguous() and y_dev.numel() == self.n, \
            "BalancePlan.order: the plan's labels as a contiguous int64 device tensor"
        order, y_out = out if out is not None else (torch.empty(self.rows, dtype=torch.int64, device=dev),
                                                    torch.empty(self.rows, dtype=torch.int64, device=dev) if want_labels else None)
        for t in (order, y_out):
            assert t is None or (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == self.rows)
        check(load().slnlp_balanced_order(self.handle, ptr(y_dev), int(seed) % (1 << 64), int(epoch), ptr(order), ptr(y_out), stream_ptr()),
              "balanced_order")
        return order, y_out

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                load().slnlp_balance_plan_destroy(h)
            except Exception:                            # interpreter shutdown: the module globals are already gone
                pass
            self.handle = None
