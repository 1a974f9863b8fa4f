"""Plain restatements of the recurrent and attention kernels' arithmetic for the kernel parity tests (test_rnn_kernels_gpu.py,
test_attn_long_gpu.py).  Everything is dtype-generic torch on the CPU: the tests run it in float64, take backward references
from autograd through these forward functions, and rerun it in float32 / with format-rounded products as yardsticks of what a
chain of timesteps may differ by.  test_kernel_refs_cpu.py pins this module to torch.nn.LSTM / GRU and to oracle.rnn_ref."""
import math

import torch


# ------------------------------------------------------------------------------------------------ recurrent cell
def cell(rnn_type, xproj, hproj, h_prev, c_prev=None):
    """torch.nn.LSTM (gates i,f,g,o) / torch.nn.GRU (r,z,n) from xproj = x W_ih^T + b_ih and hproj = h_prev W_hh^T + b_hh
    -> (h_new, c_new | None, acts [B, G*Hd], hn | None): acts are the gate activations, hn the hidden part of the n gate."""
    Hd = h_prev.shape[-1]
    if rnn_type == "lstm":
        g = xproj + hproj
        i, f = torch.sigmoid(g[:, :Hd]), torch.sigmoid(g[:, Hd:2 * Hd])
        gg, o = torch.tanh(g[:, 2 * Hd:3 * Hd]), torch.sigmoid(g[:, 3 * Hd:])
        c = f * c_prev + i * gg
        return o * torch.tanh(c), c, torch.cat([i, f, gg, o], -1), None
    r = torch.sigmoid(xproj[:, :Hd] + hproj[:, :Hd])
    z = torch.sigmoid(xproj[:, Hd:2 * Hd] + hproj[:, Hd:2 * Hd])
    hn = hproj[:, 2 * Hd:]
    n = torch.tanh(xproj[:, 2 * Hd:] + r * hn)
    return (1.0 - z) * n + z * h_prev, None, torch.cat([r, z, n], -1), hn


def step(rnn_type, xproj, hproj, h_prev, c_prev=None, valid=None, fill=0.0, keep=None, p=0.0):
    """One length-masked timestep (packed-sequence semantics): rows with valid[b] False carry their state and emit `fill`;
    live rows emit the new h through the supplied dropout keep-mask (``keep`` [B, Hd] of 0 / 1, scaled by 1 / (1 - p)).
    valid None: every row is live.  -> dict(h, c, acts, hn, out)."""
    h2, c2, acts, hn = cell(rnn_type, xproj, hproj, h_prev, c_prev)
    out = h2 if keep is None else h2 * keep / (1.0 - p)
    h, c = h2, c2
    if valid is not None:
        v = valid.unsqueeze(1)
        h = torch.where(v, h2, h_prev)
        c = None if c2 is None else torch.where(v, c2, c_prev)
        out = torch.where(v, out, torch.full_like(out, float(fill)))
    return dict(h=h, c=c, acts=acts, hn=hn, out=out)


def layer(rnn_type, xproj, w_hh, b_hh, lengths, h0, c0=None, *, fill=0.0, keep=None, p=0.0, product=None):
    """One bidirectional layer over S timesteps.  xproj / w_hh / b_hh / h0 / c0: one entry per direction (xproj[d] [S, B, G*Hd]
    time-major, direction 1 walks t = S-1 .. 0); keep [S, B, 2 Hd] or None; product(h, w) = h w^T (the recurrent product).
    -> dict: per direction the lists h / c / acts / hn / hproj indexed by time (state AFTER the step at time t), h_final /
    c_final per direction, out [S, B, 2 Hd]."""
    product = product or (lambda h, w: h @ w.T)
    S, Hd = xproj[0].shape[0], w_hh[0].shape[1]
    res = {k: [[None] * S for _ in range(2)] for k in ("h", "c", "acts", "hn", "hproj")}
    outs = [[None] * S for _ in range(2)]
    res["h_final"], res["c_final"] = [None, None], [None, None]
    for d in range(2):
        h, c = h0[d], (c0[d] if rnn_type == "lstm" else None)
        for t in (range(S) if d == 0 else range(S - 1, -1, -1)):
            hproj = product(h, w_hh[d]) + b_hh[d]
            if hproj.requires_grad:
                hproj.retain_grad()
            st = step(rnn_type, xproj[d][t], hproj, h, c, t < lengths, fill,
                      None if keep is None else keep[t][:, d * Hd:(d + 1) * Hd], p)
            h, c = st["h"], st["c"]
            for k in ("h", "c", "acts", "hn"):
                res[k][d][t] = st[k]
            res["hproj"][d][t] = hproj
            outs[d][t] = st["out"]
        res["h_final"][d], res["c_final"][d] = h, c
    res["out"] = torch.cat([torch.stack(outs[0]), torch.stack(outs[1])], -1)
    return res


# ------------------------------------------------------------------------------------------------ format yardstick
def bf16_split(x):
    """x -> (head, tail): the bf16 rounding of x and the bf16 rounding of what it leaves, in x's dtype."""
    hi = x.to(torch.bfloat16).to(x.dtype)
    return hi, (x - hi).to(torch.bfloat16).to(x.dtype)


def fmt_matmul(a, b, precision):
    """a @ b with the operands replaced by their format-rounded values: precision 3 = bf16 heads and tails without the
    tail x tail term (the three MFMA passes of the split-bf16 GEMMs), precision 1 = bf16 heads only."""
    ah, al = bf16_split(a)
    bh, bl = bf16_split(b)
    if precision == 1:
        return ah @ bh
    return ah @ bh + ah @ bl + al @ bh


class _FmtProduct(torch.autograd.Function):
    """h w^T whose forward and both backward products run through fmt_matmul."""

    @staticmethod
    def forward(ctx, h, w, precision):
        ctx.save_for_backward(h, w)
        ctx.precision = precision
        return fmt_matmul(h, w.T, precision)

    @staticmethod
    def backward(ctx, g):
        h, w = ctx.saved_tensors
        return fmt_matmul(g, w, ctx.precision), fmt_matmul(g.T, h, ctx.precision), None


def fmt_product(precision):
    return lambda h, w: _FmtProduct.apply(h, w, precision)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ one layer, forward + BPTT
def chain(rnn_type, inp, dtype=torch.float64, product=None):
    """Forward of `layer` and autograd backward of  sum dout * out + sum dh_final * h_final (+ sum dc_final * c_final)  in
    `dtype`.  inp: xproj, w_hh, b_hh (per direction), lengths, fill, keep, p, dout [S, B, 2 Hd], dh_final, dc_final (per
    direction); the initial states are zero.  -> dict of float64 tensors, per direction stacked over time: h, c, acts, out
    (forward), dgx = d/d xproj, dgh = d/d hproj, dh0, dc0 = d/d initial state."""
    lstm = rnn_type == "lstm"
    cast = lambda x: x.to(dtype)
    xproj = [cast(x.detach()).clone().requires_grad_(True) for x in inp["xproj"]]
    w_hh, b_hh = [cast(w) for w in inp["w_hh"]], [cast(b) for b in inp["b_hh"]]
    S, B = xproj[0].shape[:2]
    Hd = w_hh[0].shape[1]
    h0 = [torch.zeros(B, Hd, dtype=dtype, requires_grad=True) for _ in range(2)]
    c0 = [torch.zeros(B, Hd, dtype=dtype, requires_grad=True) for _ in range(2)] if lstm else None
    keep = None if inp["keep"] is None else cast(inp["keep"])
    r = layer(rnn_type, xproj, w_hh, b_hh, inp["lengths"], h0, c0, fill=inp["fill"], keep=keep, p=inp["p"], product=product)
    loss = (cast(inp["dout"]) * r["out"]).sum()
    for d in range(2):
        loss = loss + (cast(inp["dh_final"][d]) * r["h_final"][d]).sum()
        if lstm:
            loss = loss + (cast(inp["dc_final"][d]) * r["c_final"][d]).sum()
    loss.backward()
    out = {}
    for d in range(2):
        out[f"h{d}"] = torch.stack(r["h"][d])
        out[f"acts{d}"] = torch.stack(r["acts"][d])
        out[f"out{d}"] = r["out"][:, :, d * Hd:(d + 1) * Hd]
        out[f"dgx{d}"] = xproj[d].grad
        out[f"dh0{d}"] = h0[d].grad
        if lstm:
            out[f"c{d}"] = torch.stack(r["c"][d])
            out[f"dc0{d}"] = c0[d].grad
        else:
            out[f"dgh{d}"] = torch.stack([hp.grad for hp in r["hproj"][d]])
    return {k: v.detach().double() for k, v in out.items()}


def chain_yardsticks(rnn_type, inp, precision):
    """-> (ref, e_fp32, e_fmt): the float64 chain and, per tensor of it, the error of the same chain evaluated in float32 and
    of the float64 chain whose recurrent products run on format-rounded operands (fmt_matmul), both relative to ref."""
    ref = chain(rnn_type, inp)
    f32 = chain(rnn_type, inp, dtype=torch.float32)
    fmt = chain(rnn_type, inp, product=fmt_product(precision))
    return ref, {k: rel(f32[k], ref[k]) for k in ref}, {k: rel(fmt[k], ref[k]) for k in ref}


# ------------------------------------------------------------------------------------------------ attention
def _mha_ref(qkv, ids, pad, B, S, H, dh, causal, mask=None, p=0.0):
    """Self-attention core of one layer for any S: qkv [S*B, 3E] (q | k | v, rows time-major) -> (ctx [S*B, E], probs
    [B, H, S, S] before dropout); key j is blocked for query i where j > i (causal) or ids[b, j] == pad (ids may be None);
    mask [B, H, S, S]: dropout keep-mask on the probabilities."""
    E = H * dh
    x = qkv.view(S, B, 3, H, dh)
    q, k, v = [x[:, :, i].permute(1, 2, 0, 3) for i in range(3)]           # [B,H,S,dh]
    sc = q @ k.transpose(-1, -2) / math.sqrt(dh)
    blocked = torch.zeros(B, 1, S, S, dtype=torch.bool)
    if causal:
        blocked = blocked | torch.triu(torch.ones(S, S, dtype=torch.bool), 1)
    if ids is not None:
        blocked = blocked | (ids == pad).view(B, 1, 1, S)
    pr = torch.softmax(sc.masked_fill(blocked, float("-inf")), -1)
    pd = pr if mask is None else pr * mask / (1 - p)
    ctx = (pd @ v).permute(2, 0, 1, 3).reshape(S * B, E)
    return ctx, pr


def cross_ref(q, kv, B, S, H, dh, mask=None, p=0.0):
    """Cross-attention with one query per sequence and no masks: q [B, E], kv [S*B, 2E] (k | v, rows time-major) -> (ctx
    [B, E], probs [B, H, S] before dropout); mask [B, H, S]: dropout keep-mask on the probabilities."""
    E = H * dh
    qh = q.view(B, H, 1, dh)
    k = kv[:, :E].reshape(S, B, H, dh).permute(1, 2, 0, 3)
    v = kv[:, E:].reshape(S, B, H, dh).permute(1, 2, 0, 3)
    pr = torch.softmax(qh @ k.transpose(-1, -2) / math.sqrt(dh), -1)       # [B,H,1,S]
    pd = pr if mask is None else pr * mask.view(B, H, 1, S) / (1 - p)
    return (pd @ v).reshape(B, E), pr.view(B, H, S)
