"""The decoder's LayerNorms as the prologue of the B-row product they feed (csrc/gemm_rows.hip: gemm_rows_ln_kernel;
slnlp_gemm_rows_ln, slnlp_tf_set_dec_ln_fused, default on) against today's two launches (slnlp_layernorm_fwd, then
slnlp_gemm_rows; switch off).  The prologue runs the stand-alone kernel's row arithmetic with its lane-to-column mapping and
reductions, and the product is the B-row kernel's, so nothing may move by a bit: every comparison here is torch.equal on the
int32 view (NaN rows compare too), no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A                 # int16 pattern of plane rows nobody may write
EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _same(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ operator level
# (id, M, N, K, epilogue)
OP_CASES = [
    ("one-k-tile-one-row", 1, 16, 64, dict()),                                  # seven waves normalise but own no K tile
    ("partial-row-block", 15, 16, 64, dict(bias=True)),
    ("one-slot-half-the-lanes", 16, 48, 128, dict(bias=True)),                  # one float4 slot per lane, half the lanes past E
    ("generator", 17, 202, 512, dict(bias=True, ldc=204)),                      # N % 16 != 0, padded ldc, last row block: one live row
    ("bias-dropout-residual", 50, 512, 512, dict(bias=True, drop=0.1, resid=True)),
    ("relu-dropout-planes", 50, 256, 512, dict(bias=True, relu=1, drop=0.1, planes=True)),
    ("per-head-dropout", 50, 512, 512, dict(bias=True, drop=0.1, head_dim=64)),
    ("two-k-tiles-four-slots", 64, 512, 1024, dict(bias=True)),
]


@pytest.mark.parametrize("prec", [3, 1])
@pytest.mark.parametrize("name,M,N,K,epi", OP_CASES, ids=[c[0] for c in OP_CASES])
def test_one_launch_equals_layernorm_then_product_bit_for_bit(ops, name, M, N, K, epi, prec):
    dev = "cuda"
    x = (rnd(M, K, seed=1, scale=3.0) + 0.5).to(dev)
    gamma, beta = (1 + 0.1 * rnd(K, seed=2)).to(dev), (0.1 * rnd(K, seed=3)).to(dev)
    W = rnd(N, K, seed=4, scale=0.05).to(dev)
    bias = rnd(N, seed=5).to(dev) if epi.get("bias") else None
    resid = rnd(M, N, seed=6).to(dev) if epi.get("resid") else None
    rng = ops.make_rng(seed=7, step=3)
    ldc, Mp = epi.get("ldc", N), ops.pad64(M)
    kw = dict(M=M, N=N, K=K, precision=prec, bias=bias, relu=epi.get("relu", 0), drop_p=epi.get("drop", 0.0), drop_site=11, rng=rng,
              drop_head_dim=epi.get("head_dim", 0), resid=resid)

    # today's two launches; the planes between them as LayerNorm's plane output holds them (split_bf16 of y, zero padding)
    y_ref, st_ref = ops.layernorm_fwd(x, gamma, beta, EPS)
    yp_ref = ops.split_planes(y_ref)
    c_ref = torch.full((M, ldc), 7.0, device=dev)
    res = ops.gemm_rows(yp_ref, W, out=c_ref, want_planes=bool(epi.get("planes")), **kw)
    cp_ref = res[1] if epi.get("planes") else None

    # one launch; rows M .. of y's planes hold a sentinel and must come back unchanged, rows < M hold other garbage
    y = torch.full((M, K), float("nan"), device=dev)
    st = torch.full((M, 2), float("nan"), device=dev)
    yp = [torch.full((Mp, K), SENTINEL, dtype=torch.int16, device=dev) for _ in range(2)]
    for t in yp:
        t[:M] = 0x1234
    c = torch.full((M, ldc), 7.0, device=dev)
    cp = [torch.zeros(Mp, ops.pad64(N), dtype=torch.int16, device=dev) for _ in range(2)] if epi.get("planes") else None
    ops.gemm_rows_ln(x, gamma, beta, W, y=y, stats=st, y_planes=yp, eps=EPS, out=c, out_planes=cp, **kw)
    torch.cuda.synchronize()

    assert _same(y, y_ref), "y differs"
    assert _same(st, st_ref), "(mean, rstd) differ"
    assert _same(yp[0][:M], yp_ref[0][:M]) and _same(yp[1][:M], yp_ref[1][:M]), "y planes differ"
    assert bool((yp[0][M:] == SENTINEL).all()) and bool((yp[1][M:] == SENTINEL).all()), "plane rows >= M were written"
    assert _same(c, c_ref), "C differs"
    if cp is not None:
        assert _same(cp[0], cp_ref[0]) and _same(cp[1], cp_ref[1]), "C planes differ"
    if epi.get("drop"):
        assert bool((c[:, :N] == (resid if resid is not None else 0.0)).any()), "nothing was dropped"


def test_overlapping_x_and_y_and_unsupported_launches_are_refused(ops):
    M, N, K = 16, 32, 64
    buf = torch.zeros(2 * M * K, device="cuda")
    x = buf[:M * K].view(M, K)
    gamma = torch.ones(K, device="cuda")
    W = rnd(N, K, seed=1).cuda()
    for y in (x, buf[M * K - 4:2 * M * K - 4].view(M, K)):                       # in place; y starts inside x's last row
        with pytest.raises(RuntimeError, match="overlap"):
            ops.gemm_rows_ln(x, gamma, gamma, W, M=M, N=N, K=K, y=y)
    y = torch.empty(M, K, device="cuda")
    with pytest.raises(RuntimeError, match="overlap"):                           # a residual that is the launch's own y
        ops.gemm_rows_ln(x, gamma, gamma, rnd(K, K, seed=2).cuda(), M=M, N=K, K=K, y=y, resid=y)
    from slnlp._lib import load
    assert load().slnlp_set_rows_tile(1) == 0                                    # a forced 64 x 16 tile: not this kernel's launch
    try:
        with pytest.raises(RuntimeError, match="16 x 16"):
            ops.gemm_rows_ln(x, gamma, gamma, W, M=M, N=N, K=K, y=y)
    finally:
        assert load().slnlp_set_rows_tile(-1) == 0
    ops.gemm_rows_ln(x, gamma, gamma, W, M=M, N=N, K=K, y=y)                     # ... and apart they are taken
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ plan level
BENCH = dict(E=512, H=8, N=6, F=512, Vs=3000, Vt=202, B=50, S=48)
SMALL = dict(E=64, H=4, N=2, F=128, Vs=64, Vt=16, B=6, S=13)

# (id, shape, batch rows, dropout, put <pad> targets into the batch)
PLAN_CASES = [
    ("small-nodrop", SMALL, 6, 0.0, False),
    ("small-drop", SMALL, 6, 0.1, False),
    ("partial-batch-pad", dict(SMALL, B=8), 5, 0.1, True),
    ("one-slot-e128", dict(SMALL, E=128), 6, 0.1, False),
    ("four-slots-e1024", dict(SMALL, E=1024, H=8, N=1, S=8), 6, 0.1, False),
    ("row-block-boundary-b64", dict(SMALL, B=64), 64, 0.1, False),
    ("bench-drop", BENCH, 50, 0.1, False),
    # where the switch has (next to) nothing to switch: the results must still be equal
    ("b80-plane-gemm-decoder", dict(SMALL, B=80), 80, 0.1, False),              # rows_for false but for the per-head-dropout product
    ("e32-fp32-operands", dict(SMALL, E=32, F=64), 6, 0.1, False),              # E not a multiple of 64: no B-row products at all
]


def _engine(c, dropout, seed=100, fused=True):
    from oracle import transformer_ref as tr
    from slnlp import synth, tf_engine as te
    cfg = te.make_config(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"], c["B"], c["S"], 1, 1, dropout, 3)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_weights(tr.param_shapes(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"]), seed=10).items()}
    e = te.TransformerEngine(cfg, seed=seed)
    e.load_state(sd)
    e.set_lr(0.01)
    _set_fused(e, fused)
    return e


def _set_fused(e, on):
    from slnlp._lib import check, load
    check(load().slnlp_tf_set_dec_ln_fused(e.handle, int(on)), "tf_set_dec_ln_fused")
    e._graph_keys = {}                                   # the plan dropped its captured graphs


def _batch(c, rows, seed=50, pad=False):
    from slnlp import synth
    Xn, _, yn = synth.make_batch(rows, c["S"], c["Vs"], c["Vt"], seed=seed, min_len=min(3, c["S"]))
    X, y = torch.from_numpy(Xn).cuda(), torch.from_numpy(yn).cuda()
    if pad:
        y[1::4] = 1                                     # pad_tgt: these rows are NaN from the embedding on
    return X, y


def _assert_same_state(a, b, rows, what):
    torch.cuda.synchronize()
    assert _same(a.logp[:rows], b.logp[:rows]), f"{what}: log-probs differ"
    assert _same(a.scalars[:2], b.scalars[:2]), f"{what}: loss / grad norm differ"
    assert _same(a.grads, b.grads), f"{what}: gradient arenas differ"
    assert _same(a.params, b.params) and _same(a.momentum, b.momentum), f"{what}: parameters / momentum after the update differ"


@pytest.mark.parametrize("name,c,rows,dropout,pad", PLAN_CASES, ids=[k[0] for k in PLAN_CASES])
def test_switch_on_equals_switch_off_bit_for_bit(name, c, rows, dropout, pad):
    on, off = _engine(c, dropout, fused=True), _engine(c, dropout, fused=False)
    for step in range(2):
        X, y = _batch(c, rows, seed=50 + step, pad=pad)
        on.train_step(X, y, 0.9, 0.5)
        off.train_step(X, y, 0.9, 0.5)
        _assert_same_state(on, off, rows, f"{name} step {step}")
    assert bool((on.grads.view(torch.int32) != 0).any()), f"{name}: no gradient was written"
    X, y = _batch(c, rows, seed=59, pad=pad)
    la, lb = on.forward(X, y, train=False).clone(), off.forward(X, y, train=False).clone()
    torch.cuda.synchronize()
    assert _same(la, lb), f"{name}: eval log-probs differ"
    assert pad or bool(torch.isfinite(la).all()), f"{name}: eval log-probs are not finite"


@pytest.mark.parametrize("name,c,rows", [("bench", BENCH, 50), ("s13", SMALL, 6)])
def test_eager_launches_equal_graph_replay_with_the_switch_on(name, c, rows):
    eager, graph = _engine(c, 0.1), _engine(c, 0.1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for step in range(3):
            X, y = _batch(c, rows, seed=60 + step)
            eager.train_step(X, y, 0.9, 0.5)
            graph.train_step_graph(X, y, 0.9, 0.5)
            _assert_same_state(eager, graph, rows, f"{name} step {step}")
            if step == 0:                                # a change of the switch drops the captured graph: off and on again
                _set_fused(graph, False)
                _set_fused(graph, True)


def test_lockstep_group_equals_solo_fits_and_its_program_ignores_the_switch():
    """Three fits (own seeds and data) as one LockstepGroup against the three solo fits, switch on, then off in every fit (the group
    re-records: the settings generation moved): the solo bits both times, and the train program has the same number of launches
    -- a recorder never takes the fused kernel."""
    from slnlp.lockstep import LockstepGroup
    c = SMALL
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
                _set_fused(e, on)
            for f in range(K):
                for r in range(0, 2 * B, B):
                    solo[f].train_step(data[f][0][r:r + B], data[f][1][r:r + B], 0.9, 0.5)
            grp.epoch(0, B, True, 0.9, 0.5)
            torch.cuda.synchronize()
            counts.append(grp.num_launches(0, B, True))
            for f in range(K):
                assert _same(solo[f].grads, lock[f].grads), f"fit {f}, switch {on}: gradient arenas differ between solo and lockstep"
                assert _same(solo[f].params, lock[f].params) and _same(solo[f].momentum, lock[f].momentum)
        grp.close()
    assert counts[0] > 0 and counts[0] == counts[1], counts
