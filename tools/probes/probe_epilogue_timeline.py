"""Where the epilogue of a 96 x 64 plane-GEMM workgroup spends its time: per-workgroup 100 MHz stamps of K loop end -> drain ->
end of phase 1b -> barrier in front of phase 2 -> last store, for the three launch kinds of a cfg2 train step (M = 2400, N = 512).
Needs the timeline probe build with the epilogue stamps:

    make -C sign-language-nlp_amd PROBE=128 EXTRA=-DSLNLP_PROBE_EPI=1
    python tools/probes/probe_epilogue_timeline.py           (SLNLP_PROBE_LIB=<variant> for another probe library)

Every kind is reported back to back (operands in the L2 / Infinity Cache) and COLD: behind a pass over 1 GiB and other kernels,
with the residual / gate / bias rewritten by another kernel first, as the launch finds them inside a train step.
"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sign-language-nlp_amd")]
os.environ.setdefault("SLNLP_PROBE_LIB", "128")
import numpy as np, torch
from slnlp import ops
from slnlp._lib import load, check
lib = load()
lib.slnlp_probe_ts.restype = C.c_int
lib.slnlp_probe_ts.argtypes = [C.c_void_p, C.c_int]
buf = np.zeros((1 << 16, 8), dtype=np.uint64)   # words: gemm_planes.hip TS_W (6 / 7 = behind phase 1b / behind the barrier in front of phase 2)
TILE = int(os.environ.get("PROBE_TILE", "96"))
M, N = 2400, 512


def read():
    n = lib.slnlp_probe_ts(buf.ctypes.data, buf.shape[0])
    assert n >= 0
    return buf[:n].astype(np.int64).copy()


_big = torch.empty(256 << 20, dtype=torch.float32, device="cuda")      # 1 GiB
_other = torch.randn(4096, 512, device="cuda")
def evict(touch):
    _big.add_(1.0)
    torch.nn.functional.layer_norm(_other, (512,)); torch.softmax(_other, -1); _other @ _other.T
    for t in touch: t.mul_(1.0)                   # the epilogue's operands: last written by another kernel, from whichever XCD ran it
    torch.cuda.synchronize()


q = lambda a: "%6.2f %6.2f %6.2f" % tuple(np.percentile(a, [10, 50, 90]))
def phases(t):
    us = lambda a: a / 100.0
    return (us(t[:, 2] - t[:, 0]), us(t[:, 3] - t[:, 2]), us(t[:, 6] - t[:, 3]), us(t[:, 7] - t[:, 6]), us(t[:, 4] - t[:, 7]),
            us(t[:, 4] - t[:, 2]), us(t[:, 4] - t[:, 0]), us(t[:, 4].max() - t[:, 0].min()))


def line(tag, rows):
    p = [np.concatenate(x) if isinstance(x[0], np.ndarray) else np.array(x) for x in zip(*[phases(t) for t in rows])]
    print(f"    {tag:5s} p10/p50/p90 us: entry..K loop end {q(p[0])} | drain {q(p[1])} | 1a+1b {q(p[2])} | barrier+requests {q(p[3])} "
          f"| phase 2 to last store {q(p[4])} || after the K loop {q(p[5])} | workgroup {q(p[6])} | launch span mean {p[7].mean():6.2f}")


def report(name, launch, touch):
    check(lib.slnlp_set_plane_tile(TILE), "tile")
    for _ in range(50): launch()
    read()
    hot = []
    for _ in range(6):
        launch(); hot.append(read())
    cold = []
    for _ in range(6):
        evict(touch); read(); launch(); cold.append(read())
    print(f"{name}: tile {TILE}, {len(hot[0])} workgroups, 6 launches each")
    line("hot", hot)
    line("COLD", cold)
    check(lib.slnlp_set_plane_tile(0), "tile")


g = torch.Generator().manual_seed(0)
rnd = lambda *s: torch.randn(*s, generator=g).cuda()
rng = ops.make_rng(seed=7, step=5)


def forward(K):
    """out_proj / linear2: three passes, bias, dropout, residual, fp32 store + planes."""
    X, W, bias, R = rnd(M, K), rnd(N, K), rnd(N), rnd(M, N)
    Xp, Wp = ops.split_planes(X), ops.split_planes(W)
    j, Y = ops.plane_job(Xp, Wp, M=M, N=N, K=K, bias=bias, resid=R)
    j.drop_p, j.drop_site, j.rng = 0.1, 3, rng.data_ptr()
    cp = ops.split_planes(torch.zeros(M, N).cuda())
    j.C_hi, j.C_lo, j.ldc_p = cp[0].data_ptr(), cp[1].data_ptr(), cp[0].stride(0)
    scr = ops.gemm_group([j], [1])
    return (lambda: ops.gemm_group([j], [1], scr)), [bias, R], (X, W, Xp, Wp, Y, cp)


def dgrad(K, which):
    """two-pass data gradient (dY's bf16 head): + residual (linear1 / in_proj), or ReLU gate with scale (linear2)."""
    dY, W, R = rnd(M, K), rnd(K, N), rnd(M, N)
    dYp, Wp = ops.split_planes(dY), ops.split_planes(W)
    j, dX = ops.plane_job(dYp, Wp, M=M, N=N, K=K, b_kmajor=False, precision=2, resid=R if which == "resid" else None)
    if which == "gate":
        j.gate, j.ldg, j.gate_scale, j.gate_mode = R.data_ptr(), R.stride(0), 1.0 / 0.9, 0
    scr = ops.gemm_group([j], [1])
    return (lambda: ops.gemm_group([j], [1], scr)), [R], (dY, W, dYp, Wp, dX)


for name, (launch, touch, keep) in (
        ("forward K=512, three passes, bias + dropout + residual + planes", forward(512)),
        ("data gradient K=512, two passes, + residual                    ", dgrad(512, "resid")),
        ("data gradient K=512, two passes, ReLU gate                      ", dgrad(512, "gate")),
        ("data gradient K=1536, two passes, + residual                   ", dgrad(1536, "resid"))):
    report(name, launch, touch)
