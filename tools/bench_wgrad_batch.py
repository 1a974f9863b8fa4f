"""The two halves of the encoder's gradient pairs apart, at the cfg2 shapes (2400 tokens; E x E pairs: split-K 3, in_proj pairs:
no split): device time of (a) the pair as ONE launch (slnlp_gemm_wd: what a train step launched before the weight gradients
left the chain), (b) the data gradient alone (what stays on the chain), (c) weight-gradient jobs merged into one launch -- four
per launch, the most the public grouped entry takes (MAX_JOBS); the plan's own batched launch holds all 24 in one table-driven
launch and is read off a kernel trace of the train step instead (profiles/r06_bench_cfg2_kernel_trace_summary.txt) -- at each
tile geometry.  Every figure back to back (operands warm in the L2s) and cold (a 1 GiB write between launches).

    python tools/bench_wgrad_batch.py
"""
import ctypes as C
import sys
import torch
sys.path.insert(0, "sign-language-nlp_amd")
from slnlp import ops
from slnlp._lib import load, check

TOK = 2400
wp, dp = C.c_int32(0), C.c_int32(0)
check(load().slnlp_get_backward_passes(C.byref(wp), C.byref(dp)), "get_backward_passes")
WPASS, DPASS = wp.value, dp.value
evict = torch.empty(1 << 28, dtype=torch.float32, device="cuda")       # 1 GiB: larger than every cache on the package
keep = []


def warm_us(fn, n=200, warm=20):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def cold_us(fn, n=12):
    ts = []
    for _ in range(n):
        evict.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def pair(Nout, Kin, seed):
    g = torch.Generator().manual_seed(seed)
    dY, X, W = [torch.randn(*s, generator=g).cuda() for s in ((TOK, Nout), (TOK, Kin), (Nout, Kin))]
    dYp, Xp, Wp = ops.split_planes(dY), ops.split_planes(X), ops.split_planes(W)
    rs = torch.empty(Nout, device="cuda")
    jw, dW = ops.plane_job(dYp, Xp, M=Nout, N=Kin, K=TOK, a_kmajor=False, b_kmajor=False, rowsum_a=rs, precision=WPASS)
    jd, dX = ops.plane_job(dYp, Wp, M=TOK, N=Kin, K=Nout, a_kmajor=True, b_kmajor=False, precision=DPASS)
    keep.append((dYp, Xp, Wp, rs, dW, dX))
    return jw, jd


print(f"passes: wgrad {WPASS}, dgrad {DPASS}; {TOK} tokens; us per launch, back to back / cold (median of 12 behind a 1 GiB write)")
total = {}
for name, Nout, Kin, count in (("E x E pair   512 x 512", 512, 512, 18), ("in_proj pair 1536 x 512", 1536, 512, 6)):
    jobs = [pair(Nout, Kin, s) for s in range(4)]
    jw, jd = jobs[0]
    split, separate, _, _ = ops.gemm_wd_plan(jw, jd)
    assert not separate
    scr = ops.gemm_wd(jw, jd)
    a = (warm_us(lambda: ops.gemm_wd(jw, jd, scr)), cold_us(lambda: ops.gemm_wd(jw, jd, scr)))
    b = (warm_us(lambda: ops.gemm_group([jd], [1], scr)), cold_us(lambda: ops.gemm_group([jd], [1], scr)))
    print(f"{name}  split {split}  x{count} per step")
    print(f"  (a) pair, one launch          {a[0]:7.1f} / {a[1]:7.1f} us")
    print(f"  (b) data gradient alone       {b[0]:7.1f} / {b[1]:7.1f} us      (a) - (b) = {a[0] - b[0]:6.1f} / {a[1] - b[1]:6.1f} us")
    wj, ws = [j[0] for j in jobs], [split] * 4
    scr4 = ops.gemm_group(wj, ws)
    for tile in (64, 128, 12832):
        check(load().slnlp_set_plane_tile(tile), "set_plane_tile")
        c = (warm_us(lambda: ops.gemm_group(wj, ws, scr4)), cold_us(lambda: ops.gemm_group(wj, ws, scr4)))
        check(load().slnlp_set_plane_tile(0), "set_plane_tile")
        print(f"  (c) 4 weight gradients, one launch, tile {tile:5d}: {c[0]:7.1f} / {c[1]:7.1f} us   = {c[0] / 4:5.1f} / {c[1] / 4:5.1f} us per job")
        total.setdefault(tile, [0.0, 0.0])
        total[tile][0] += c[0] / 4 * count; total[tile][1] += c[1] / 4 * count
    total.setdefault("saved", [0.0, 0.0])
    total["saved"][0] += (a[0] - b[0]) * count; total["saved"][1] += (a[1] - b[1]) * count
print(f"per step: sum of (a) - (b) over the 24 pairs  {total['saved'][0]:7.1f} / {total['saved'][1]:7.1f} us")
for tile in (64, 128, 12832):
    print(f"          24 weight gradients at tile {tile:5d}  {total[tile][0]:7.1f} / {total[tile][1]:7.1f} us   "
          f"net {total['saved'][0] - total[tile][0]:7.1f} / {total['saved'][1] - total[tile][1]:7.1f} us")
