"""Pins tests/kernel_refs.py, the fp64 reference of the kernel parity tests, to independent implementations: torch.nn.LSTM /
GRU over packed sequences (outputs, final states and every gradient to 1e-12) and oracle.rnn_ref.run_direction; and pins the
format yardstick the chain tests scale their bounds with."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import kernel_refs as kr


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
@pytest.mark.parametrize("B,S,In,Hd,fill", [(6, 7, 5, 8, 1.0), (3, 4, 9, 12, 0.0), (9, 5, 4, 6, -2.5)])
def test_bidirectional_ragged_layer_equals_torch_packed_rnn(rnn_type, B, S, In, Hd, fill):
    lstm = rnn_type == "lstm"
    g = torch.Generator().manual_seed(B * 100 + S + lstm)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    net = (torch.nn.LSTM if lstm else torch.nn.GRU)(In, Hd, batch_first=True, bidirectional=True).double()
    for prm in net.parameters():
        prm.data = rnd(*prm.shape) * 0.4
    lengths = torch.randint(1, S + 1, (B,), generator=g)
    lengths[0], lengths[1] = 1, S
    assert int(lengths.min()) == 1 and int(lengths.max()) == S
    x = rnd(B, S, In).requires_grad_(True)
    h0 = rnd(2, B, Hd).requires_grad_(True)
    c0 = rnd(2, B, Hd).requires_grad_(True)
    w_out, w_h, w_c = rnd(B, S, 2 * Hd), rnd(2, B, Hd), rnd(2, B, Hd)

    packed = pack_padded_sequence(x, lengths, batch_first=True, enforce_sorted=False)
    y, hid = net(packed, (h0, c0) if lstm else h0)
    y, _ = pad_packed_sequence(y, batch_first=True, padding_value=fill, total_length=S)
    hn, cn = hid if lstm else (hid, None)
    loss = (w_out * y).sum() + (w_h * hn).sum() + ((w_c * cn).sum() if lstm else 0.0)
    leaves = [x, h0] + ([c0] if lstm else []) + list(net.parameters())
    grads_t = torch.autograd.grad(loss, leaves)

    sfx = ["", "_reverse"]
    prm = lambda name, d: getattr(net, f"{name}_l0{sfx[d]}")
    xproj = [(x @ prm("weight_ih", d).T + prm("bias_ih", d)).transpose(0, 1) for d in range(2)]
    r = kr.layer(rnn_type, xproj, [prm("weight_hh", d) for d in range(2)], [prm("bias_hh", d) for d in range(2)], lengths,
                 [h0[0], h0[1]], [c0[0], c0[1]], fill=fill)
    y2 = r["out"].transpose(0, 1)
    loss2 = (w_out * y2).sum() + sum((w_h[d] * r["h_final"][d]).sum() for d in range(2))
    if lstm:
        loss2 = loss2 + sum((w_c[d] * r["c_final"][d]).sum() for d in range(2))
    grads_r = torch.autograd.grad(loss2, leaves)

    assert kr.rel(y2, y) < 1e-12
    assert torch.all(y2[torch.arange(S)[None, :] >= lengths[:, None]] == fill)
    assert kr.rel(torch.stack(r["h_final"]), hn) < 1e-12
    if lstm:
        assert kr.rel(torch.stack(r["c_final"]), cn) < 1e-12
    names = ["x", "h0"] + (["c0"] if lstm else []) + [n for n, _ in net.named_parameters()]
    for n, a, b in zip(names, grads_r, grads_t):
        assert float(b.abs().max()) > 0, n
        assert kr.rel(a, b) < 1e-12, n


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_masked_single_step_equals_oracle_run_direction(rnn_type):
    from oracle import rnn_ref
    B, In, Hd = 7, 5, 6
    G = 4 if rnn_type == "lstm" else 3
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {"weight_ih": rnd(G * Hd, In), "weight_hh": rnd(G * Hd, Hd), "bias_ih": rnd(G * Hd), "bias_hh": rnd(G * Hd)}
    x = rnd(B, 1, In)
    lengths = torch.tensor([1, 0, 1, 1, 0, 1, 0])
    out_o, h_o = rnn_ref.run_direction(x, lengths, sd, "", "", rnn_type, False)
    z = torch.zeros(B, Hd, dtype=torch.float64)
    xproj = x[:, 0] @ sd["weight_ih"].T + sd["bias_ih"]
    st = kr.step(rnn_type, xproj, z @ sd["weight_hh"].T + sd["bias_hh"], z, z, valid=0 < lengths, fill=0.0)
    assert torch.equal(st["out"], out_o[:, 0]) and torch.equal(st["h"], h_o)
    assert torch.all(st["h"][lengths == 0] == 0) and float(st["h"][lengths == 1].abs().min()) > 0
    # valid=None is the all-live step; a keep-mask scales live outputs by 1 / (1 - p) and leaves the state alone
    keep = (torch.rand(B, Hd, generator=g) > 0.3).double()
    live = kr.step(rnn_type, xproj, z @ sd["weight_hh"].T + sd["bias_hh"], z, z, keep=keep, p=0.3)
    full = kr.step(rnn_type, xproj, z @ sd["weight_hh"].T + sd["bias_hh"], z, z, valid=torch.ones(B, dtype=torch.bool))
    assert torch.equal(live["h"], full["h"]) and torch.equal(live["out"], full["h"] * keep / 0.7)


def test_format_yardstick():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(40, 96, generator=g, dtype=torch.float64)
    b = torch.randn(96, 24, generator=g, dtype=torch.float64)
    hi, lo = kr.bf16_split(a)
    assert torch.equal(hi, a.to(torch.bfloat16).double()) and float((a - hi - lo).abs().max()) < 2.0 ** -15 * float(a.abs().max())
    exact = a @ b
    e3, e1 = kr.rel(kr.fmt_matmul(a, b, 3), exact), kr.rel(kr.fmt_matmul(a, b, 1), exact)
    print(f"format yardstick: precision 3 {e3:.2e}, precision 1 {e1:.2e}")
    assert 0 < e3 < e1
    assert e3 < 5e-5 and 1e-4 < e1 < 2e-2          # inside the project's single-product classes (TOL of test_kernels_gpu.py)
    # the autograd function runs forward and both backward products on rounded operands
    h, w = a.clone().requires_grad_(True), b.T.clone().requires_grad_(True)
    y = kr.fmt_product(3)(h, w)
    assert torch.equal(y, kr.fmt_matmul(a, b, 3))
    gy = torch.randn(40, 24, generator=g, dtype=torch.float64)
    y.backward(gy)
    assert torch.equal(h.grad, kr.fmt_matmul(gy, b.T, 3)) and torch.equal(w.grad, kr.fmt_matmul(gy.T, a, 3))
    assert kr.rel(h.grad, gy @ b.T) < 5e-5


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_chain_yardsticks_are_small_ordered_and_finite(rnn_type):
    B, Hd, S = 5, 8, 6
    G = 4 if rnn_type == "lstm" else 3
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    inp = dict(xproj=[rnd(S, B, G * Hd) for _ in range(2)], w_hh=[rnd(G * Hd, Hd) * 0.3 for _ in range(2)],
               b_hh=[rnd(G * Hd) * 0.1 for _ in range(2)], lengths=torch.tensor([1, S, 3, 2, S]), fill=1.0,
               keep=(torch.rand(S, B, 2 * Hd, generator=g) > 0.2).double(), p=0.2, dout=rnd(S, B, 2 * Hd),
               dh_final=[rnd(B, Hd) for _ in range(2)], dc_final=[rnd(B, Hd) for _ in range(2)])
    ref, e32, e3 = kr.chain_yardsticks(rnn_type, inp, 3)
    _, _, e1 = kr.chain_yardsticks(rnn_type, inp, 1)
    for k, v in ref.items():
        assert torch.isfinite(v).all() and float(v.abs().max()) > 0, k
        assert e32[k] < 1e-5 and e3[k] < 1e-4 and e3[k] < e1[k] < 1e-1, (k, e32[k], e3[k], e1[k])


def _keep_mask(B, S, H, p, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B * H, S, generator=g) >= p).double()


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("B,S,H,dh", kr.XMEM_SHAPES)
def test_xmem_ref_equals_the_projected_cross_attention_and_its_autograd(B, S, H, dh, p):
    """xmem_ref, with the per-head products around it, is nn.MultiheadAttention's arithmetic re-associated: forward and every
    gradient agree with cross_ref on the projected memory to 1e-12, under a dropout mask too, and d bk is zero."""
    inp = kr.xmem_block_inputs(B, S, H, dh)
    mask = _keep_mask(B, S, H, p, 31 + S) if p > 0 else None
    std = kr.xmem_block_standard(inp, B, S, H, dh, mask, p)
    got = kr.xmem_block_reassociated(inp, B, S, H, dh, mask, p)
    for k in ("ctx", "probs", "dq", "dmem", "dWk", "dWv", "dbv"):
        if S == 1 and k in ("dq", "dWk"):                               # a softmax over one element passes no gradient
            assert float(std[k].abs().max()) < 1e-12 and float(got[k].abs().max()) < 1e-12, k
            continue
        assert float(std[k].abs().max()) > 0, k
        e = kr.rel(got[k], std[k])
        print(f"xmem_ref vs standard form {(B, S, H, dh)} p={p} {k}: {e:.2e}")
        assert e < 1e-12, (k, e)
    assert float(std["dbk"].abs().max()) < 1e-12 * float(std["dbv"].abs().max())      # the kernels write no d bk: there is none
    x = got["x"]
    if p > 0:
        assert float((x["psum"] - 1).abs().max()) > 0.05                 # the mask is live: sum_s p_s != 1
    else:
        assert float((x["psum"] - 1).abs().max()) < 1e-14
    if S == 1:
        assert torch.equal(x["probs"], torch.ones_like(x["probs"])) and torch.equal(x["dsc"], torch.zeros_like(x["dsc"]))


@pytest.mark.parametrize("B,S,H,dh", [s for s in kr.XMEM_SHAPES if s[1] > 1])
def test_xmem_parity_inputs_see_the_bias_term_under_dropout(B, S, H, dh):
    """The GPU parity tests' inputs (xmem_inputs: unit-scale bv) must keep  d ctx_h . bv_h  visible: at p = 0.25, d score
    without that term differs by more than 1e-2 of its scale.  Without dropout the term cancels exactly."""
    inp = {k: v.double() for k, v in kr.xmem_inputs(B, S, H, dh).items()}
    mask = _keep_mask(B, S, H, 0.25, 5 + S)
    nobias = dict(inp, bv=torch.zeros_like(inp["bv"]))                   # bv reaches d score through that term alone
    full = kr.xmem_ref(B=B, S=S, H=H, dh=dh, mask=mask, p=0.25, **inp)
    cut = kr.xmem_ref(B=B, S=S, H=H, dh=dh, mask=mask, p=0.25, **nobias)
    e = kr.rel(cut["dsc"], full["dsc"])
    print(f"d score without d ctx . bv {(B, S, H, dh)}: {e:.3f} of its scale")
    assert e > 1e-2
    assert float((full["psum"] - 1).abs().max()) > 0.05
    assert kr.rel(kr.xmem_ref(B=B, S=S, H=H, dh=dh, **nobias)["dsc"], kr.xmem_ref(B=B, S=S, H=H, dh=dh, **inp)["dsc"]) < 1e-12
    sc = full["sc"]
    assert 0.5 < float(sc.std()) < 2.0                                   # scores near N(0, 1): neither flat nor one-hot
