"""Plain restatements of the recurrent and attention kernels' arithmetic for the kernel parity tests (test_rnn_kernels_gpu.py,
test_attn_long_gpu.py, test_attn_mem_gpu.py).  Everything is dtype-generic torch on the CPU: the tests run it in float64, take
backward references from autograd through these forward functions, and rerun it in float32 / with format-rounded products as
yardsticks of what a chain of timesteps may differ by.  test_kernel_refs_cpu.py pins this module to torch.nn.LSTM / GRU, to
oracle.rnn_ref and, for the re-associated cross-attention (xmem_ref), to autograd through the projected form (cross_ref)."""
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


def planes_are_the_split_of(planes, x):
    """hi / lo planes (int16 bit patterns) == bf16_split(x), as bf16 bit patterns."""
    hi, lo = bf16_split(x.detach().cpu())
    return (torch.equal(planes[0].cpu(), hi.to(torch.bfloat16).view(torch.int16))
            and torch.equal(planes[1].cpu(), lo.to(torch.bfloat16).view(torch.int16)))


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
def _mha_ref(qkv, ids, pad, B, S, H, dh, causal, mask=None, p=0.0, product=torch.matmul):
    """Self-attention core of one layer for any S: qkv [S*B, 3E] (q | k | v, rows time-major) -> (ctx [S*B, E], probs
    [B, H, S, S] before dropout); key j is blocked for query i where j > i (causal) or ids[b, j] == pad (ids may be None);
    mask [B, H, S, S]: dropout keep-mask on the probabilities.  ``product(a, b)`` stands for a @ b in the two contractions
    (and, through autograd, in their gradients): tests/attention_ref.py runs them on format-rounded operands."""
    E = H * dh
    x = qkv.view(S, B, 3, H, dh)
    q, k, v = [x[:, :, i].permute(1, 2, 0, 3) for i in range(3)]           # [B,H,S,dh]
    sc = product(q, k.transpose(-1, -2)) / math.sqrt(dh)
    blocked = torch.zeros(B, 1, S, S, dtype=torch.bool)
    if causal:
        blocked = blocked | torch.triu(torch.ones(S, S, dtype=torch.bool), 1)
    if ids is not None:
        blocked = blocked | (ids == pad).view(B, 1, 1, S)
    pr = torch.softmax(sc.masked_fill(blocked, float("-inf")), -1)
    pd = pr if mask is None else pr * mask / (1 - p)
    ctx = product(pd, v).permute(2, 0, 1, 3).reshape(S * B, E)
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


def xmem_ref(qk, mem, bv, dmbar, dctx, B, S, H, dh, mask=None, p=0.0):
    """Cross-attention over the unprojected memory (csrc/attention_mem.hip, header comment), every kernel output by name.
    qk [B*H, E] = Wk_h^T q_h, mem [S*B, E] (rows time-major), bv [E], dmbar [B*H, E] = Wv_h^T d ctx_h, dctx [B, E]; mask
    [B*H, S]: dropout keep-mask (0 / 1) on the probabilities, row b*H + h.  -> dict: probs, psum, mbar, ctx0 (forward; ctx =
    Wv_h mbar + ctx0), dsc, dqk, dcp, dbv, dmem (backward), and sc, pd, t (intermediates)."""
    E = H * dh
    m = mem.view(S, B, E).transpose(0, 1)                                  # [B,S,E]
    q3, g3 = qk.view(B, H, E), dmbar.view(B, H, E)
    keep = torch.ones(B, H, S, dtype=qk.dtype) if mask is None else mask.view(B, H, S).to(qk.dtype) / (1 - p)
    sc = torch.einsum("bhe,bse->bhs", q3, m) / math.sqrt(dh)
    probs = torch.softmax(sc, -1)
    pd = probs * keep
    psum = pd.sum(-1)                                                      # [B,H]
    mbar = torch.einsum("bhs,bse->bhe", pd, m)
    ctx0 = (bv.view(1, H, dh) * psum.unsqueeze(-1)).reshape(B, E)
    c = (dctx.view(B, H, dh) * bv.view(1, H, dh)).sum(-1)                  # d ctx_h . bv_h
    t = (torch.einsum("bhe,bse->bhs", g3, m) + c.unsqueeze(-1)) * keep
    dsc = probs * (t - (probs * t).sum(-1, keepdim=True)) / math.sqrt(dh)
    dqk = torch.einsum("bhs,bse->bhe", dsc, m)
    dcp = (dctx.view(B, H, dh) * psum.unsqueeze(-1)).reshape(B, E)
    dbv = dcp.sum(0)
    dmem = (torch.einsum("bhs,bhe->sbe", pd, g3) + torch.einsum("bhs,bhe->sbe", dsc, q3)).reshape(S * B, E)
    return dict(sc=sc.reshape(B * H, S), probs=probs.reshape(B * H, S), pd=pd.reshape(B * H, S), psum=psum.reshape(B * H),
                mbar=mbar.reshape(B * H, E), ctx0=ctx0, t=t.reshape(B * H, S), dsc=dsc.reshape(B * H, S),
                dqk=dqk.reshape(B * H, E), dcp=dcp, dbv=dbv, dmem=dmem)


XMEM_SHAPES = [(3, 13, 3, 8), (5, 70, 4, 16), (2, 1, 2, 4), (4, 27, 1, 64)]   # (B, S, H, dh) the CPU pins and the GPU parity tests share


def xmem_inputs(B, S, H, dh, seed=0):
    """float32 inputs of the memory cross-attention kernels as the parity tests draw them: everything at unit scale, bv
    included, but qk at sqrt(dh / E) per element, so that the scores are roughly N(0, 1): a softmax neither flat nor one-hot."""
    E = H * dh
    g = torch.Generator().manual_seed(1000 * seed + 97 * B + 13 * S + 7 * H + dh)
    rnd = lambda *s: torch.randn(*s, generator=g)
    return dict(qk=rnd(B * H, E) * math.sqrt(dh / E), mem=rnd(S * B, E), bv=rnd(E), dmbar=rnd(B * H, E), dctx=rnd(B, E))


def xmem_block_inputs(B, S, H, dh, seed=0):
    """float32 inputs of the whole block in its standard form: q [B, E], mem [S*B, E], the K and V blocks of in_proj (Wk, Wv
    [E, E] at 1 / sqrt(E), the scale that keeps q . k / sqrt(dh) near N(0, 1)), unit-scale biases bk, bv [E] and dctx [B, E]."""
    E = H * dh
    g = torch.Generator().manual_seed(2000 * seed + 97 * B + 13 * S + 7 * H + dh)
    rnd = lambda *s: torch.randn(*s, generator=g)
    return dict(q=rnd(B, E), mem=rnd(S * B, E), Wk=rnd(E, E) / math.sqrt(E), Wv=rnd(E, E) / math.sqrt(E), bk=rnd(E), bv=rnd(E),
                dctx=rnd(B, E))


def xmem_block_standard(inp, B, S, H, dh, mask=None, p=0.0):
    """The block as nn.MultiheadAttention computes it, in float64: cross_ref on kv = [mem Wk^T + bk | mem Wv^T + bv] and autograd
    of sum(ctx * dctx).  -> dict: ctx, probs, dq, dmem, dWk, dWv, dbk, dbv."""
    E = H * dh
    leaf = {k: inp[k].double().clone().requires_grad_(True) for k in ("q", "mem", "Wk", "Wv", "bk", "bv")}
    kv = torch.cat([leaf["mem"] @ leaf["Wk"].T + leaf["bk"], leaf["mem"] @ leaf["Wv"].T + leaf["bv"]], 1)
    ctx, probs = cross_ref(leaf["q"], kv, B, S, H, dh, None if mask is None else mask.double().view(B, H, S), p)
    grads = torch.autograd.grad((ctx * inp["dctx"].double()).sum(), [leaf[k] for k in ("q", "mem", "Wk", "Wv", "bk", "bv")])
    out = dict(zip(("dq", "dmem", "dWk", "dWv", "dbk", "dbv"), grads))
    out.update(ctx=ctx.detach(), probs=probs.detach().reshape(B * H, S))
    return out


def xmem_block_reassociated(inp, B, S, H, dh, mask=None, p=0.0):
    """The same block the way the plan runs it, in float64: the per-head products as einsums around xmem_ref.  -> dict as
    xmem_block_standard's (no dbk: the re-associated form has none), plus qk, dmbar and xmem_ref's own outputs under "x"."""
    E = H * dh
    d = {k: v.double() for k, v in inp.items()}
    Wk, Wv = d["Wk"].view(H, dh, E), d["Wv"].view(H, dh, E)
    qk = torch.einsum("bhd,hde->bhe", d["q"].view(B, H, dh), Wk).reshape(B * H, E)
    dmbar = torch.einsum("bhd,hde->bhe", d["dctx"].view(B, H, dh), Wv).reshape(B * H, E)
    x = xmem_ref(qk, d["mem"], d["bv"], dmbar, d["dctx"], B, S, H, dh, None if mask is None else mask.double(), p)
    ctx = torch.einsum("bhe,hde->bhd", x["mbar"].view(B, H, E), Wv).reshape(B, E) + x["ctx0"]
    dq = torch.einsum("bhe,hde->bhd", x["dqk"].view(B, H, E), Wk).reshape(B, E)
    dWk = torch.einsum("bhd,bhe->hde", d["q"].view(B, H, dh), x["dqk"].view(B, H, E)).reshape(E, E)
    dWv = torch.einsum("bhd,bhe->hde", d["dctx"].view(B, H, dh), x["mbar"].view(B, H, E)).reshape(E, E)
    return dict(ctx=ctx, probs=x["probs"], dq=dq, dmem=x["dmem"], dWk=dWk, dWv=dWv, dbv=x["dbv"], qk=qk, dmbar=dmbar, x=x)
