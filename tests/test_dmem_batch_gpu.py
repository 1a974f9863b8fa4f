"""The decoder backward's gradient with respect to the encoder memory, all layers in one launch behind the layer loop
(csrc/attention_mem.hip: xmem_dmem_all_kernel; slnlp_tf_set_dmem_batched, default on) against a launch per layer inside the loop
(switch off).  The merged kernel starts from zero and walks the layers N-1 ... 0 and the heads 0 ... H-1 inside each: per element
the fp32 operations of the per-layer launches in their order.  So nothing may move by a bit: every comparison here is torch.equal
on the int32 view (NaN rows compare too), no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BENCH = dict(E=512, H=8, N=6, F=512, Vs=3000, Vt=202, B=50, S=48)
SMALL = dict(E=64, H=4, N=2, F=128, Vs=64, Vt=16, B=6, S=13)          # S not a multiple of the kernel's 8 rows per workgroup

# (id, shape, batch rows, dropout, put a <pad> target into the batch)
CASES = [
    ("bench-drop", BENCH, 50, 0.1, False),
    ("bench-nodrop", BENCH, 50, 0.0, False),
    ("s13-h4-n2", SMALL, 6, 0.1, False),
    ("s13-nodrop-pad", SMALL, 6, 0.0, True),
    ("partial-batch-pad", dict(SMALL, B=8), 5, 0.1, True),
    ("n1-h8", dict(SMALL, N=1, H=8, S=48), 6, 0.1, False),             # nothing to accumulate
    ("n9", dict(SMALL, E=32, F=64, N=9, S=20), 6, 0.1, False),         # more layers than one staging trip of the kernel holds
    ("s72-long-attention", dict(SMALL, S=72, B=4), 4, 0.1, False),
    ("e32-fp32-operands", dict(SMALL, E=32, F=64), 6, 0.1, False),     # E not a multiple of 64: the fp32-operand decoder path
]


def _engine(c, dropout, seed=100):
    from oracle import transformer_ref as tr
    from slnlp import synth, tf_engine as te
    cfg = te.make_config(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"], c["B"], c["S"], 1, 1, dropout, 3)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_weights(tr.param_shapes(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"]), seed=10).items()}
    e = te.TransformerEngine(cfg, seed=seed)
    e.load_state(sd)
    e.set_lr(0.01)
    return e


def _batch(c, rows, seed=50, pad=False):
    from slnlp import synth
    Xn, _, yn = synth.make_batch(rows, c["S"], c["Vs"], c["Vt"], seed=seed, min_len=min(3, c["S"]))
    X, y = torch.from_numpy(Xn).cuda(), torch.from_numpy(yn).cuda()
    if pad:
        y[1::4] = 1                                     # pad_tgt
    return X, y


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_same_state(a, b, rows, what):
    S, E = a.cfg.S, a.cfg.E
    da, db = a.tap("dmemory", S * rows, E), b.tap("dmemory", S * rows, E)
    torch.cuda.synchronize()
    assert bool((da.view(torch.int32) != 0).any()), f"{what}: d memory was never written"       # (NaN after a <pad> target counts)
    assert _same(da, db), f"{what}: d memory differs"
    assert _same(a.grads, b.grads), f"{what}: gradient arenas differ"
    assert _same(a.logp[:rows], b.logp[:rows]), f"{what}: log-probs differ"
    assert _same(a.scalars[:2], b.scalars[:2]), f"{what}: loss / grad norm differ"
    assert _same(a.params, b.params) and _same(a.momentum, b.momentum), f"{what}: parameters after the update differ"


@pytest.mark.parametrize("name,c,rows,dropout,pad", CASES, ids=[k[0] for k in CASES])
def test_one_launch_for_all_layers_equals_a_launch_per_layer_bit_for_bit(name, c, rows, dropout, pad):
    on, off = _engine(c, dropout), _engine(c, dropout)
    off.set_dmem_batched(False)
    for step in range(2):
        X, y = _batch(c, rows, seed=50 + step, pad=pad)
        on.train_step(X, y, 0.9, 0.5)
        off.train_step(X, y, 0.9, 0.5)
        _assert_same_state(on, off, rows, f"{name} step {step}")
    # every layer's d bv (the value rows of the cross-attention in_proj bias) was written by the merged launch
    gv = on.views(on.grads)
    for l in range(c["N"]):
        db = gv[f"transformer.decoder.layers.{l}.multihead_attn.in_proj_bias"][2 * c["E"]:]
        assert bool((db.view(torch.int32) != 0).any()), f"{name}: layer {l} d bv was never written"


@pytest.mark.parametrize("name,c,rows", [("bench", BENCH, 50), ("s13", SMALL, 6)])
def test_eager_launches_equal_graph_replay_with_the_switch_on(name, c, rows):
    eager, graph = _engine(c, 0.1), _engine(c, 0.1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for step in range(3):
            X, y = _batch(c, rows, seed=60 + step)
            eager.train_step(X, y, 0.9, 0.5)
            graph.train_step_graph(X, y, 0.9, 0.5)
            torch.cuda.synchronize()
            _assert_same_state(eager, graph, rows, f"{name} step {step}")
            if step == 0:                                # a change of the switch drops the captured graph: off and on again
                graph.set_dmem_batched(False)
                graph.set_dmem_batched(True)


def test_lockstep_group_equals_solo_fits_and_drops_five_call_sites():
    """Three fits (own seeds and data) as one LockstepGroup against the three solo fits, switch on; then the same group with the
    switch off in every fit (the group re-records: the settings generation moved): still the solo bits, and the train program
    has exactly N - 1 = 5 more launches."""
    from slnlp.lockstep import LockstepGroup
    c = dict(SMALL, N=6)
    B, K = c["B"], 3
    data = [_batch(c, 2 * B, seed=70 + f) for f in range(K)]
    solo = [_engine(c, 0.1, seed=200 + f) for f in range(K)]
    lock = [_engine(c, 0.1, seed=200 + f) for f in range(K)]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        grp = LockstepGroup(lock)
        grp.set_data(0, [d[0] for d in data], [d[1] for d in data], B)
        counts = []
        for on in (True, False):
            for e in solo + lock:
                e.set_dmem_batched(on)
            for f in range(K):
                for r in range(0, 2 * B, B):
                    solo[f].train_step(data[f][0][r:r + B], data[f][1][r:r + B], 0.9, 0.5)
            grp.epoch(0, B, True, 0.9, 0.5)
            torch.cuda.synchronize()
            counts.append(grp.num_launches(0, B, True))
            for f in range(K):
                assert _same(solo[f].grads, lock[f].grads), f"fit {f}, switch {on}: gradient arenas differ between solo and lockstep"
                assert _same(solo[f].params, lock[f].params) and _same(solo[f].momentum, lock[f].momentum)
                assert _same(solo[f].tap("dmemory", c["S"] * B, c["E"]), lock[f].tap("dmemory", c["S"] * B, c["E"]))
        grp.close()
    assert counts[0] > 0 and counts[1] - counts[0] == c["N"] - 1, counts
