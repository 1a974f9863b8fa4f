"""The encoder's weight gradients off the backward chain (csrc/tf_plan.hpp: enc_pair_launch / build_wbatch): a solo plan runs the
data gradients alone inside the layer loop and all deferred weight gradients in one batched launch behind it; a lockstep
recorder keeps the paired launches.  Every deferred job keeps the split factor of its pair, so nothing may move by a bit:
everything here is torch.equal, no tolerance."""
import ctypes as C

import pytest
import torch

import gold

pytestmark = pytest.mark.gpu


def _engine(c, dropout, seed=100, B=None):
    from oracle import transformer_ref as tr
    from slnlp import synth, tf_engine as te
    cfg = te.make_config(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"], B or c["B"], c["S"], 1, 1, dropout, 3)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_weights(tr.param_shapes(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"]), seed=10).items()}
    e = te.TransformerEngine(cfg, seed=seed)
    e.load_state(sd)
    e.set_lr(0.01)
    return e


def _batch(c, rows, seed=50):
    from slnlp import synth
    Xn, _, yn = synth.make_batch(rows, c["S"], c["Vs"], c["Vt"], seed=seed, min_len=c["min_len"])
    return torch.from_numpy(Xn).cuda(), torch.from_numpy(yn).cuda()


def _plane_tap(e, name, rows, cols):
    """(hi, lo) int16 planes [rows, cols] of a GEMM operand as the kernels read it (slnlp_tf_tap "enc<l>.<planes>")."""
    raw = e.tap(name, rows, cols)                      # rows * cols floats = two planes of 16-bit words
    w = raw.view(torch.int16).view(2, rows, cols)
    return w[0], w[1]


def _padded(planes, rows):
    from slnlp.ops import pad64
    out = []
    for p in planes:
        q = torch.zeros(pad64(rows), p.shape[1], dtype=torch.int16, device=p.device)
        q[:rows] = p[:rows]
        out.append(q)
    return tuple(out)


@pytest.mark.parametrize("name", ["tiny", "cfg1", "cfg2"])
def test_batched_weight_gradients_equal_the_paired_launches_bit_for_bit(name):
    """One train step (dropout on) through the solo plan -- batched weight gradients where the shapes defer them -- against
    the same weights / batch / seed stepped as a ONE-fit LockstepGroup, whose recorder keeps the paired launches: the whole
    gradient arena and the updated parameters.  Then, for encoder layer 0, the public paired entry (ops.gemm_wd) on the very
    planes the plan's kernels read must return the dW / db bits that sit in the plan's arena."""
    from slnlp import ops
    from slnlp.lockstep import LockstepGroup
    g, c, sd, X, L, y = gold.tf_case(name)
    B, S, E = c["B"], c["S"], c["E"]
    Xd, yd = _batch(c, B)
    solo, lock = _engine(c, 0.1), _engine(c, 0.1)
    solo.train_step(Xd, yd, 0.9, 0.5)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        grp = LockstepGroup([lock])
        grp.set_data(0, [Xd], [yd], B)
        grp.epoch(0, B, True, 0.9, 0.5)
        torch.cuda.synchronize()
    grp.close()
    assert torch.equal(solo.grads, lock.grads), f"{name}: gradient arenas differ between batched and paired weight gradients"
    assert torch.equal(solo.params, lock.params) and torch.equal(solo.momentum, lock.momentum)
    assert float(solo.grads.abs().max()) > 0
    # ---- layer 0's in_proj and out_proj pairs through the public paired entry, on the tapped operand planes
    if E % 64 or c["F"] % 64:
        return                                        # (no plane GEMMs at this shape: fp32-operand pairs, nothing deferred)
    from slnlp._lib import load, check
    wp, dp = C.c_int32(0), C.c_int32(0)
    check(load().slnlp_get_backward_passes(C.byref(wp), C.byref(dp)), "get_backward_passes")
    M = S * B
    gv = solo.views(solo.grads)
    pre = "transformer.encoder.layers.0.self_attn."
    for dy_tap, x_tap, nout, wname, bname in (("enc0.gqkvp", "enc0.xinp", 3 * E, pre + "in_proj_weight", pre + "in_proj_bias"),
                                              ("enc0.d1p", "enc0.ctxp", E, pre + "out_proj.weight", pre + "out_proj.bias")):
        dYp, Xp = _padded(_plane_tap(solo, dy_tap, M, nout), M), _padded(_plane_tap(solo, x_tap, M, E), M)
        Wp = ops.split_planes(torch.zeros(nout, E, device="cuda"))       # (the data gradient's weight: its dX is not compared)
        db = torch.empty(nout, device="cuda")
        jw, dW = ops.plane_job(dYp, Xp, M=nout, N=E, K=M, a_kmajor=False, b_kmajor=False, rowsum_a=db, precision=wp.value)
        jd, dX = ops.plane_job(dYp, Wp, M=M, N=E, K=nout, a_kmajor=True, b_kmajor=False, precision=dp.value)
        ops.gemm_wd(jw, jd)
        torch.cuda.synchronize()
        assert torch.equal(dW, gv[wname]), f"{name}: {wname} gradient differs from the paired public entry"
        assert torch.equal(db, gv[bname]), f"{name}: {bname} gradient differs from the paired public entry"


@pytest.mark.parametrize("name", ["cfg1", "cfg2"])
def test_eager_and_graph_replayed_steps_give_identical_parameters(name):
    g, c, sd, X, L, y = gold.tf_case(name)
    B = c["B"]
    Xd, yd = _batch(c, 3 * B)
    eager, graph = _engine(c, 0.1), _engine(c, 0.1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for r in range(0, 3 * B, B):
            eager.train_step(Xd[r:r + B], yd[r:r + B], 0.9, 0.5)
            graph.train_step_graph(Xd[r:r + B], yd[r:r + B], 0.9, 0.5)
        torch.cuda.synchronize()
    assert torch.equal(eager.params, graph.params) and torch.equal(eager.grads, graph.grads)
    assert torch.equal(eager.momentum, graph.momentum)


@pytest.mark.parametrize("name", ["cfg1", "cfg2"])
def test_batch_size_changes_rebuild_the_job_table(name):
    """B -> B // 3 + 1 -> B rows (cfg2: 50 -> 17 -> 50; the job table, its split factors and scratch regions follow the batch
    size): after every step the plan's gradient arena equals that of a FRESH plan (same weights, momentum, rng) that has only
    ever seen this batch size, and a graph-replayed twin equals the eager plan."""
    g, c, sd, X, L, y = gold.tf_case(name)
    B = c["B"]
    small = B // 3 + 1
    sizes = [B, small, B]
    Xd, yd = _batch(c, sum(sizes))
    eager, graph = _engine(c, 0.1), _engine(c, 0.1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        r = 0
        for n in sizes:
            xb, yb = Xd[r:r + n], yd[r:r + n]
            fresh = _engine(c, 0.1)
            fresh.params.copy_(eager.params); fresh.momentum.copy_(eager.momentum); fresh.rng.copy_(eager.rng)
            eager.train_step(xb, yb, 0.9, 0.5)
            graph.train_step_graph(xb, yb, 0.9, 0.5)
            fresh.train_step(xb, yb, 0.9, 0.5)
            torch.cuda.synchronize()
            assert torch.equal(eager.grads, fresh.grads), f"{name}: batch {n}: a plan that changed its batch size differs from a fresh one"
            assert torch.equal(eager.grads, graph.grads) and torch.equal(eager.params, graph.params), f"{name}: batch {n}: eager / graph"
            r += n
