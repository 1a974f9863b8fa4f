"""GPU parity of the recurrent kernels -- slnlp_rnn_cell_fwd / _bwd, slnlp_rnn_step_fwd / _bwd, slnlp_rnn_layer_fwd,
slnlp_bahdanau_fwd / _bwd -- through the C ABI against fp64 restatements of the same operations (tests/kernel_refs.py,
oracle/rnn_ref.py), backward references by fp64 autograd.  No test here compares a kernel with another kernel.

Tolerances (max|got - ref| / max|ref| per tensor, printed per case): single kernels in fp32 arithmetic 2e-5, the class of
exact-fp32 kernels in test_kernels_gpu.py.  A chain of S timesteps has no such class: its bound is measured on the references
at run time, 4 x (e_fmt + e_fp32) floored at 2e-5, where e_fp32 is the reference chain evaluated in torch float32 and e_fmt the
float64 chain with every recurrent product on format-rounded operands (kernel_refs.chain_yardsticks) -- the yardsticks are one
sample of random rounding and the kernels add in another order, hence the factor 4."""
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

TOL_FP32 = 2e-5
COND = 2e-6               # torch float32 against fp64 on a cell test's inputs: the inputs must leave fp32 this margin
CHAIN_FACTOR = 4.0


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    return o


def _finite(tensors):
    assert all(torch.isfinite(t).all() for t in tensors), "a reference tensor is not finite"


def _site_mask(ops, rows, cols, p, site, blocks, seed=3):
    """Dumped keep-mask [rows, cols] of a dropout site whose every block (row slice, column slice) has kept and dropped
    elements: the rng step is advanced until the mask qualifies (tiny blocks can come out all kept)."""
    for step in range(1, 200):
        rng = ops.make_rng(seed=seed, step=step)
        m = ops.dropout_mask(rows, cols, p, site, rng).cpu()
        if all(0 < float(m[r, c].sum()) < m[r, c].numel() for r, c in blocks):
            return rng, m
    raise AssertionError("no rng step gives every block kept and dropped elements")


# =============================================================================== cell forward + backward, one timestep
CELL_SHAPES = [(50, 512), (7, 40), (1, 4), (70, 64), (300, 1024)]          # the last: > 1 grid-stride trip at the 1024-block cap


def _cell_case(ops, lstm, ndir, B, Hd, p, scale, mode="masked", n_extra=0):
    from slnlp._lib import RnnCellBwdDir, RnnCellDir
    rnn_type, G = ("lstm", 4) if lstm else ("gru", 3)
    GH, t, fill, site, ld = G * Hd, 2, 1.0, 40, 2 * Hd
    g = torch.Generator().manual_seed(1000 * B + Hd + 7 * lstm + ndir)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
    if mode == "no_lengths":                                               # the decoder step
        length_sets = [None]
    elif B == 1:                                                           # one row is masked or live: one launch of each
        length_sets = [torch.tensor([1]), torch.tensor([5])]
    else:
        length_sets = [torch.randint(1, 6, (B,), generator=g)]
    if mode != "no_lengths":
        allv = torch.cat([t < L for L in length_sets])
        assert allv.any() and not allv.all()                               # masked and live rows both occur
    stride = B * Hd + 24                                                   # extra_stride > B * Hd
    # gate pre-activations (xproj + hproj) of std `scale`, except every fourth hidden unit, which stays at std 1: a tensor
    # whose every element is saturated has a cancellation residue for its scale, and no fp32 evaluation of these formulas meets
    # a relative bound on it (torch float32 on a 4-unit row at scale 4: 5e-5 of fp64) -- asserted below as COND
    col_scale = torch.where(torch.arange(Hd) % 4 == 0, 1.0, float(scale)).repeat(G) / 2 ** 0.5
    for lengths in length_sets:
        valid = None if lengths is None else (t < lengths)
        live = torch.ones(B, dtype=torch.bool) if valid is None else valid
        rng, keep_site = None, None
        if p > 0:
            rows = live.nonzero().flatten() + t * B
            blocks = [(rows, slice(k * Hd, (k + 1) * Hd)) for k in range(ndir)] if len(rows) else []
            rng, keep_site = _site_mask(ops, (t + 1) * B, ndir * Hd, p, site, blocks)
        out = None if mode == "no_out" else torch.full((B, ld), 7.0).cuda()
        dout_all = rnd(B, ld)
        fdirs, bdirs, dev, ref = [], [], [], []
        for k in range(ndir):
            x = dict(xproj=rnd(B, GH) * col_scale, hproj=rnd(B, GH) * col_scale, h=rnd(B, Hd) * 0.5, c=rnd(B, Hd) * 0.5,
                     dh=rnd(B, Hd), dc=rnd(B, Hd), extra=rnd(max(n_extra, 1), stride))
            keep = None if keep_site is None else keep_site[t * B:(t + 1) * B, k * Hd:(k + 1) * Hd]

            def reference(dt):    # forward, then autograd of  sum dh . h_after + sum dc . c_after + sum dout . out
                leaves = {n: x[n].to(dt).requires_grad_(True) for n in ("xproj", "hproj", "h", "c")}
                st = kr.step(rnn_type, leaves["xproj"], leaves["hproj"], leaves["h"], leaves["c"] if lstm else None, valid, fill,
                             None if keep is None else keep.to(dt), p)
                dh_tot = x["dh"].to(dt) + x["extra"][:n_extra, :B * Hd].to(dt).reshape(n_extra, B, Hd).sum(0)
                loss = (dh_tot * st["h"]).sum()
                if lstm:
                    loss = loss + (x["dc"].to(dt) * st["c"]).sum()
                if out is not None:
                    loss = loss + (dout_all[:, k * Hd:(k + 1) * Hd].to(dt) * st["out"]).sum()
                loss.backward()
                grad = {n: (torch.zeros_like(l) if l.grad is None else l.grad) for n, l in leaves.items()}   # None: on no path
                return st, leaves, grad, dh_tot

            st, leaves, grad, dh_tot = reference(torch.float64)
            _finite([v for v in st.values() if v is not None] + list(grad.values()))
            st32, _, grad32, _ = reference(torch.float32)                  # the premise of the 2e-5 class: fp32 is 10 x inside it
            for n, a, b in [(n, st32[n], st[n]) for n in st if st[n] is not None] + [(n, grad32[n], grad[n]) for n in grad]:
                assert kr.rel(a, b) < COND, f"inputs ill-conditioned for fp32: {n} {kr.rel(a, b):.1e}"
            ref.append((st, leaves, grad, dh_tot))
            # ---- device buffers
            d = {n: v.cuda() for n, v in x.items()}
            d.update(hprev=torch.zeros(B, Hd).cuda(), cprev=torch.zeros(B, Hd).cuda(), acts=torch.zeros(B, GH).cuda(),
                     hn=torch.zeros(B, Hd).cuda(), dgx=torch.full((B, GH), 9.0).cuda(), dgh=torch.full((B, GH), 9.0).cuda(),
                     carry=torch.full((B, Hd), 9.0).cuda(), dout=dout_all.cuda(), dc0=x["dc"].cuda())
            dev.append(d)
            fdirs.append(ops.dir_struct(RnnCellDir, xproj=d["xproj"], hproj=d["hproj"], h=d["h"], c=d["c"], hprev_save=d["hprev"],
                                        cprev_save=d["cprev"], acts=d["acts"], hn_save=d["hn"],
                                        out=None if out is None else out[:, k * Hd:], t=t, out_row0=t * B, out_col0=k * Hd))
            bdirs.append(ops.dir_struct(RnnCellBwdDir, dh_state=d["dh"], dc_state=d["dc"],
                                        dout=None if out is None else d["dout"][:, k * Hd:], acts=d["acts"], cprev_save=d["cprev"],
                                        hprev_save=d["hprev"], hn_save=d["hn"], dgx=d["dgx"], dgh=None if lstm else d["dgh"],
                                        carry=d["carry"], t=t, out_row0=t * B, out_col0=k * Hd,
                                        dh_extra=d["extra"] if n_extra else None, extra_stride=stride, n_extra=n_extra))
        L = None if lengths is None else lengths.cuda()
        ops.rnn_cell_fwd(lstm, fdirs, B=B, Hd=Hd, lengths=L, fill=fill, ld_out=ld, drop_p=p, drop_site=site, rng=rng)
        ops.rnn_cell_bwd(lstm, bdirs, B=B, Hd=Hd, lengths=L, ld_dout=ld, drop_p=p, drop_site=site, rng=rng)
        torch.cuda.synchronize()
        errs = {}
        for k in range(ndir):
            d, (st, leaves, grad, dh_tot) = dev[k], ref[k]
            x_h, x_c = leaves["h"].detach(), leaves["c"].detach()
            errs[f"h{k}"] = kr.rel(d["h"], st["h"])
            errs[f"acts{k}"] = kr.rel(d["acts"], st["acts"])
            assert torch.equal(d["hprev"].cpu().double(), x_h)             # the saves are copies, masked rows included
            if lstm:
                errs[f"c{k}"] = kr.rel(d["c"], st["c"])
                assert torch.equal(d["cprev"].cpu().double(), x_c)
            else:
                errs[f"hn{k}"] = kr.rel(d["hn"], st["hn"])
            if out is not None:
                errs[f"out{k}"] = kr.rel(out[:, k * Hd:(k + 1) * Hd], st["out"])
                assert torch.all(out[~live.cuda(), k * Hd:(k + 1) * Hd] == fill)
            errs[f"dgx{k}"] = kr.rel(d["dgx"], grad["xproj"])
            errs[f"carry{k}"] = kr.rel(d["carry"], grad["h"])
            if lstm:
                errs[f"dc{k}"] = kr.rel(d["dc"], grad["c"])
                assert torch.all(d["carry"][live.cuda()] == 0)             # LSTM: no direct path from h_prev on live rows
            else:
                errs[f"dgh{k}"] = kr.rel(d["dgh"], grad["hproj"])
            masked = (~live).cuda()
            if masked.any():                                                # gate gradients exactly zero, dc_state bit-unchanged,
                assert torch.all(d["dgx"][masked] == 0)                     # carry the whole dh
                assert lstm or torch.all(d["dgh"][masked] == 0)
                assert torch.equal(d["dc"][masked], d["dc0"][masked])
                assert kr.rel(d["carry"][masked], dh_tot[~live]) < TOL_FP32
        if out is not None and ndir == 1:
            assert torch.all(out[:, Hd:] == 7.0)                            # the other direction's columns stay untouched
        tag = f"cell {rnn_type} ndir{ndir} B{B} Hd{Hd} p{p} scale{scale} {mode} n_extra{n_extra}"
        print(tag + ": " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v < TOL_FP32, (tag, k, v)


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("B,Hd", CELL_SHAPES)
@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("lstm", [1, 0])
def test_cell_fwd_bwd_vs_fp64(ops, lstm, ndir, B, Hd, p, scale):
    """t = 2 with lengths from 1..5 (masked and live rows, asserted; the one-row shape runs one launch of each), fill 1.0,
    ld_out = 2 Hd with direction 1 at column Hd, the dropout mask dumped over the whole site at (t B, k Hd), gate
    pre-activations at scales 1 and 4 (the saturated end; every fourth hidden unit stays at scale 1, see _cell_case)."""
    _cell_case(ops, lstm, ndir, B, Hd, p, scale)


@pytest.mark.parametrize("mode", ["no_lengths", "no_out"])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("B,Hd", [(50, 512), (7, 40), (1, 4)])
@pytest.mark.parametrize("lstm", [1, 0])
def test_cell_without_lengths_and_without_out(ops, lstm, B, Hd, p, mode):
    """lengths = NULL (the decoder step: every row live) and out = NULL (no layer output, no d out)."""
    _cell_case(ops, lstm, 2, B, Hd, p, 1.0, mode=mode)


@pytest.mark.parametrize("n_extra", [0, 3, 8, 15, 17])
@pytest.mark.parametrize("B,Hd", [(50, 512), (7, 40)])
@pytest.mark.parametrize("lstm", [1, 0])
def test_cell_bwd_dh_extra_partial_sums(ops, lstm, B, Hd, n_extra):
    """dh = dh_state + sum of n_extra slices at extra_stride > B Hd: none, the plan's 3, one register block, 15, and 17 (the
    tail loop for e >= 16); the reference adds the same slices in fp64."""
    _cell_case(ops, lstm, 2, B, Hd, 0.2, 1.0, n_extra=n_extra)


# =============================================================================== one bidirectional layer, S steps, BPTT
def _after(slots, final, d, S):
    """[S, ...] state AFTER the step at time t from the chained per-timestep slots (slot t = state BEFORE time t)."""
    if d == 0:
        return torch.cat([slots[1:], final.unsqueeze(0)])
    return torch.cat([final.unsqueeze(0), slots[:-1]])


def _bound(e_fmt, e_fp32):
    return max(CHAIN_FACTOR * (e_fmt + e_fp32), TOL_FP32)


@pytest.mark.parametrize("prec", [3, 1])
@pytest.mark.parametrize("B,Hd,S,full", [(50, 512, 12, False), (7, 64, 9, False), (70, 128, 5, False), (33, 192, 6, False),
                                         (5, 40, 7, False), (7, 64, 9, True)])
@pytest.mark.parametrize("lstm", [1, 0])
def test_layer_bptt_vs_fp64_autograd(ops, lstm, B, Hd, S, full, prec):
    """Forward with S launches of slnlp_rnn_step_fwd (and, where covered, the one launch of slnlp_rnn_layer_fwd), backward with
    the chain the plan runs (slnlp_rnn_step_bwd where Hd % 64 == 0, else slnlp_rnn_cell_bwd + slnlp_gemm), dropout 0.2 on the
    layer output, ragged lengths that include 1 and S (one case all-full), against fp64 autograd through kernel_refs.layer fed
    the same masks.  Every tensor's bound is 4 x (e_fmt + e_fp32) of that tensor, floored at 2e-5 (module docstring)."""
    import ctypes as C
    from slnlp._lib import RnnCellBwdDir, RnnLayerDir, RnnStepBwdDir, RnnStepDir, check, load, ptr, stream_ptr
    rnn_type, G = ("lstm", 4) if lstm else ("gru", 3)
    GH, p, site, fill, ld = G * Hd, 0.2, 33, 1.0, 2 * Hd
    g = torch.Generator().manual_seed(B + Hd + S + lstm)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
    lengths = torch.full((B,), S) if full else torch.randint(1, S + 1, (B,), generator=g)
    if not full:
        lengths[0], lengths[1] = 1, S
        for t in range(1, S):
            assert (t < lengths).any() and not (t < lengths).all()          # masked and live rows at every step after the first
    rng, keep = _site_mask(ops, S * B, 2 * Hd, p, site, [(slice(None), slice(d * Hd, (d + 1) * Hd)) for d in range(2)])
    inp = dict(xproj=[rnd(S, B, GH) for _ in range(2)], w_hh=[rnd(GH, Hd) / Hd ** 0.5 for _ in range(2)],
               b_hh=[rnd(GH) * 0.1 for _ in range(2)], lengths=lengths, fill=fill, keep=keep.view(S, B, 2 * Hd), p=p,
               dout=rnd(S, B, 2 * Hd), dh_final=[rnd(B, Hd) for _ in range(2)], dc_final=[rnd(B, Hd) for _ in range(2)])
    ref, e_fp32, e_fmt = kr.chain_yardsticks(rnn_type, inp, prec)
    _finite(ref.values())
    W, bh, xp = [w.cuda() for w in inp["w_hh"]], [b.cuda() for b in inp["b_hh"]], [x.cuda() for x in inp["xproj"]]
    Lc = lengths.cuda()

    def buffers():
        return [dict(hprev=torch.zeros(S, B, Hd).cuda(), h=torch.zeros(B, Hd).cuda(), c=torch.zeros(B, Hd).cuda(),
                     cprev=torch.zeros(S, B, Hd).cuda(), acts=torch.zeros(S, B, GH).cuda(), hn=torch.zeros(S, B, Hd).cuda())
                for _ in range(2)]

    def forward_tensors(f, out):
        got = {}
        for d in range(2):
            got[f"h{d}"] = _after(f[d]["hprev"], f[d]["h"], d, S)
            got[f"acts{d}"] = f[d]["acts"]
            got[f"out{d}"] = out.view(S, B, 2 * Hd)[:, :, d * Hd:(d + 1) * Hd]
            if lstm:
                got[f"c{d}"] = _after(f[d]["cprev"], f[d]["c"], d, S)
        return got

    # ---- forward: one launch per timestep
    f, out = buffers(), torch.zeros(S * B, ld).cuda()
    for step in range(S):
        dirs = []
        for d in range(2):
            t = step if d == 0 else S - 1 - step
            tn = t + 1 if d == 0 else t - 1
            e = f[d]
            dirs.append(ops.dir_struct(RnnStepDir, h_in=e["hprev"][t], h_out=e["hprev"][tn] if step + 1 < S else e["h"], w_hh=W[d],
                                       b_hh=bh[d], xproj=xp[d][t], c=e["c"], cprev_save=e["cprev"][t], acts=e["acts"][t],
                                       hn_save=e["hn"][t], out=out[t * B:, d * Hd:], t=t, out_row0=t * B, out_col0=d * Hd))
        ops.rnn_step_fwd(lstm, dirs, B=B, Hd=Hd, lengths=Lc, fill=fill, ld_out=ld, drop_p=p, drop_site=site, rng=rng, precision=prec)
    torch.cuda.synchronize()
    got = forward_tensors(f, out)
    valid = (torch.arange(S)[:, None] < lengths[None, :]).cuda()            # [S, B]
    assert torch.all(out.view(S, B, ld)[~valid] == fill)

    # ---- forward: the persistent layer (B <= 64, Hd % 64 == 0, W_hh slice fits the LDS), else launched == 0 by contract
    pf, pout = buffers(), torch.zeros(S * B, ld).cuda()
    sync = torch.zeros(4, dtype=torch.int32).cuda()
    ldirs = (RnnLayerDir * 2)(*[ops.dir_struct(RnnLayerDir, hprev=pf[d]["hprev"], h_final=pf[d]["h"], w_hh=W[d], b_hh=bh[d], xproj=xp[d],
                                               c=pf[d]["c"], cprev=pf[d]["cprev"], acts=pf[d]["acts"], hn=pf[d]["hn"],
                                               out=pout[:, d * Hd:], out_col0=d * Hd, reverse=d) for d in range(2)])
    launched = C.c_int32(-1)
    check(load().slnlp_rnn_layer_fwd(lstm, ldirs, 2, B, Hd, S, ptr(Lc), fill, ld, p, site, ptr(rng), prec, ptr(sync),
                                     C.byref(launched), stream_ptr()), "layer")
    torch.cuda.synchronize()
    assert launched.value == int(B <= 64 and Hd % 64 == 0)
    assert sync.tolist()[0] == 0 and sync.tolist()[2] == 0                  # barrier at rest, no spin timeout
    pgot = forward_tensors(pf, pout) if launched.value else {}

    # ---- backward through time
    dout = inp["dout"].view(S * B, 2 * Hd).cuda()
    bw = [dict(dh=inp["dh_final"][d].cuda(), dc=inp["dc_final"][d].cuda(), carry=torch.zeros(B, Hd).cuda(),
               dgx=torch.zeros(S, B, GH).cuda(), dgh=torch.zeros(S, B, GH).cuda()) for d in range(2)]
    dgh_of = lambda d: bw[d]["dgx"] if lstm else bw[d]["dgh"]
    fused = Hd % 64 == 0
    for step in range(S - 1, -1, -1):
        cells, ts = [], []
        for d in range(2):
            t = step if d == 0 else S - 1 - step
            ts.append(t)
            e, b = f[d], bw[d]
            cells.append(dict(dh_state=b["dh"], dc_state=b["dc"], dout=dout[t * B:, d * Hd:], acts=e["acts"][t], cprev_save=e["cprev"][t],
                              hprev_save=e["hprev"][t], hn_save=e["hn"][t], dgx=b["dgx"][t], dgh=None if lstm else b["dgh"][t],
                              carry=b["carry"], t=t, out_row0=t * B, out_col0=d * Hd))
        kw = dict(B=B, Hd=Hd, lengths=Lc, ld_dout=ld, drop_p=p, drop_site=site, rng=rng)
        sdirs = []
        for d in range(2):
            tn = ts[d] + 1 if d == 0 else ts[d] - 1                        # the step processed just before
            first = step == S - 1
            sdirs.append(RnnStepBwdDir(ops.dir_struct(RnnCellBwdDir, **cells[d]), None if first else dgh_of(d)[tn].data_ptr(),
                                       None if first else W[d].data_ptr()))
        if fused:
            ops.rnn_step_bwd(lstm, sdirs, precision=prec, **kw)
            continue
        if step == S - 1:                                                   # the contract: Hd % 64 != 0 is rejected, not mis-run
            with pytest.raises(RuntimeError, match="rnn_step_bwd: bad args"):
                ops.rnn_step_bwd(lstm, sdirs, precision=prec, **kw)
        ops.rnn_cell_bwd(lstm, [ops.dir_struct(RnnCellBwdDir, **c) for c in cells], **kw)
        for d in range(2):                                                  # dh_state(t - 1) = dgh W_hh + carry
            ops.gemm(dgh_of(d)[ts[d]], W[d], M=B, N=Hd, K=GH, a_kmajor=True, b_kmajor=False, resid=bw[d]["carry"], out=bw[d]["dh"],
                     precision=prec)
    torch.cuda.synchronize()
    for d in range(2):
        t0 = 0 if d == 0 else S - 1                                         # the first timestep of the direction
        got[f"dgx{d}"] = bw[d]["dgx"]
        got[f"dh0{d}"] = dgh_of(d)[t0].double().cpu() @ inp["w_hh"][d].double() + bw[d]["carry"].double().cpu()
        if lstm:
            got[f"dc0{d}"] = bw[d]["dc"]
        else:
            got[f"dgh{d}"] = bw[d]["dgh"]
        assert torch.all(bw[d]["dgx"][~valid] == 0) and torch.all(dgh_of(d)[~valid] == 0)
    assert set(got) == set(ref)

    tag = f"bptt {rnn_type} prec{prec} B{B} Hd{Hd} S{S} {'full' if full else 'ragged'} {'fused' if fused else 'cell+gemm'}"
    failed = []
    for path, tensors in (("stepwise", got), ("persistent", pgot)):
        for k in sorted(tensors):
            err, bound = kr.rel(tensors[k], ref[k]), _bound(e_fmt[k], e_fp32[k])
            print(f"{tag} {path} {k}: err {err:.2e} e_fmt {e_fmt[k]:.2e} e_fp32 {e_fp32[k]:.2e} bound {bound:.2e}")
            if not err < bound:
                failed.append((path, k, err, bound))
    assert not failed, (tag, failed)


# =============================================================================== Bahdanau attention
def _bahdanau_inputs(B, S, Hd, lengths):
    g = torch.Generator().manual_seed(B + S + Hd)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
    ids = torch.full((B, S), 5, dtype=torch.long)
    ids[torch.arange(S)[None, :] >= lengths[:, None]] = 1
    return dict(q=rnd(B, Hd), pk=rnd(B, S, Hd), val=rnd(B, S, 2 * Hd), we=rnd(Hd) / Hd ** 0.5 * 3, dctx=rnd(B, 2 * Hd)), ids


def _bahdanau_ref(x, ids, Hd):
    """oracle.rnn_ref.bahdanau in fp64 (the query arrives projected: query_layer = identity) + autograd of sum dctx . ctx."""
    from oracle import rnn_ref
    lv = {k: x[k].double().requires_grad_(True) for k in ("q", "pk", "val", "we")}
    sd = {"model.decoder.attention.query_layer.weight": torch.eye(Hd, dtype=torch.float64),
          "model.decoder.attention.energy_layer.weight": lv["we"].view(1, Hd)}
    ctx, alphas = rnn_ref.bahdanau(lv["q"].unsqueeze(1), lv["pk"], lv["val"], (ids != 1).unsqueeze(1), sd)
    return lv, ctx.squeeze(1), alphas.squeeze(1)


def _bahdanau_gpu(ops, x, ids, B, S, Hd):
    tm = lambda a: a.transpose(0, 1).reshape(S * B, -1).contiguous().cuda()     # [B, S, C] -> time-major rows s * B + b
    q, pk, val, we = x["q"].cuda(), tm(x["pk"]), tm(x["val"]), x["we"].cuda()
    alphas, ctx = ops.bahdanau_fwd(q, pk, val, we, ids.cuda(), 1, B=B, S=S, Hd=Hd)
    grads = ops.bahdanau_bwd(q, pk, val, we, alphas, x["dctx"].cuda(), B=B, S=S, Hd=Hd)
    again = ops.bahdanau_fwd(q, pk, val, we, ids.cuda(), 1, B=B, S=S, Hd=Hd) + ops.bahdanau_bwd(q, pk, val, we, alphas, x["dctx"].cuda(),
                                                                                               B=B, S=S, Hd=Hd)
    torch.cuda.synchronize()
    for a, b in zip((alphas, ctx) + grads, again):                              # two calls are bit-identical (NaN included)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    bm = lambda a: a.view(S, B, -1).transpose(0, 1)                             # back to [B, S, C]
    dq, dpk, dval, dwe = grads
    return dict(alphas=alphas, ctx=ctx, dq=dq, dpk=bm(dpk), dval=bm(dval), dwe=dwe)


@pytest.mark.parametrize("B,S,Hd", [(50, 48, 512), (4, 65, 40), (3, 2048, 64), (2, 1, 8), (5, 300, 100)])
def test_bahdanau_fwd_bwd_vs_fp64(ops, B, S, Hd):
    """S across the 64-lane softmax stride and at BAH_MAXS, Hd off 64; pad masks from ragged lengths, no sequence fully padded."""
    g = torch.Generator().manual_seed(S)
    lengths = torch.randint(1, S + 1, (B,), generator=g)
    lengths[0] = S
    if S > 1:
        lengths[1] = max(1, S // 3)
    x, ids = _bahdanau_inputs(B, S, Hd, lengths)
    pad = ids == 1
    assert not pad.all(1).any() and (S == 1 or pad.any())
    lv, ctx_ref, al_ref = _bahdanau_ref(x, ids, Hd)
    (x["dctx"].double() * ctx_ref).sum().backward()
    refs = dict(alphas=al_ref, ctx=ctx_ref, dq=lv["q"].grad, dpk=lv["pk"].grad, dval=lv["val"].grad, dwe=lv["we"].grad)
    _finite(refs.values())
    got = _bahdanau_gpu(ops, x, ids, B, S, Hd)
    errs = {k: kr.rel(got[k], refs[k]) for k in refs}
    print(f"bahdanau B{B} S{S} Hd{Hd}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k in ("alphas", "dpk", "dval"):                                        # masked positions: exactly 0
        assert torch.all(got[k].cpu()[pad] == 0), k
    for k, v in errs.items():
        assert v < TOL_FP32, (k, v)


def test_bahdanau_fully_padded_sequence_is_nan_for_that_sequence_only(ops):
    B, S, Hd = 4, 70, 24
    lengths = torch.tensor([S, 0, 9, 33])
    x, ids = _bahdanau_inputs(B, S, Hd, lengths)
    assert (ids[1] == 1).all()
    _, ctx_ref, al_ref = _bahdanau_ref(x, ids, Hd)
    got = _bahdanau_gpu(ops, x, ids, B, S, Hd)
    alphas, ctx = got["alphas"].cpu(), got["ctx"].cpu()
    assert torch.isnan(al_ref[1]).all() and torch.isnan(alphas[1]).all()       # softmax over no position: NaN like torch
    ok = torch.tensor([0, 2, 3])
    assert not torch.isnan(alphas[ok]).any() and not torch.isnan(ctx[ok]).any()
    assert kr.rel(alphas[ok], al_ref[ok]) < TOL_FP32 and kr.rel(ctx[ok], ctx_ref[ok]) < TOL_FP32
