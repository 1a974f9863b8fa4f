"""What weight averaging costs on one MI355X: the accumulator alone, and a cfg2 train step with and without it.

    python tools/time_weight_averaging.py [--out FILE] [--tree DIR] [--no-averaging]

* ``slnlp_average_step`` at the cfg2 arena size, warm, HIP events around each of 40 calls (median), and the fraction of the
  HBM peak its 12 B per parameter reach (read avg, read params, write avg).
* one cfg2 train step (batch 50 x 48, dropout 0.1), eager and as a captured graph, averaging off and riding every step
  (``every="batch"``, EMA): 24 samples of 10 steps each between HIP events, median per step.
``--tree DIR --no-averaging`` times another checkout (the commit before the option existed) with the same code on the same
card; the two outputs are put side by side in profiles/weight_averaging_timing.json.  No pass / fail: numbers are recorded."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--no-averaging", action="store_true")
args = ap.parse_args()
for p in (args.tree, os.path.join(args.tree, "sign-language-nlp_amd")):
    sys.path.insert(0, p)

import numpy as np
import torch

CFG2 = dict(E=512, H=8, N=6, F=512, Vs=3000, Vt=202, B=50, S=48, dropout=0.1)
HBM_PEAK = 8.0e12           # bytes / s, MI355X
SAMPLES, STEPS, WARM = 24, 10, 10


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_us": float(np.median(v)), "min_us": float(v.min()), "max_us": float(v.max()), "samples": int(v.size)}


def timed(fn, samples, per):
    us = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / per)
    return us


def main():
    import bench
    from slnlp import synth, tf_engine as te
    out = {"tree": os.path.abspath(args.tree), "device": torch.cuda.get_device_name(0)}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        cfg, sd = bench.build_sd(CFG2, seed=1)
        X, L, y = (torch.from_numpy(a).cuda() for a in synth.make_batch(CFG2["B"], CFG2["S"], CFG2["Vs"], CFG2["Vt"], seed=1))

        def engine(averaging):
            e = te.TransformerEngine(cfg, device="cuda", seed=1)
            e.load_state(sd)
            e.set_lr(0.01)
            if averaging:
                e.set_averaging(torch.zeros_like(e.params), torch.zeros(1, device="cuda"), kind="ema", decay=0.999)
            return e
        modes = [("off", False)] + ([] if args.no_averaging else [("batch", True)])
        steps = {}
        for name, av in modes:
            for how in ("eager", "graph"):
                e = engine(av)
                fn = (lambda: e.train_step_graph(X, y)) if how == "graph" else (lambda: e.train_step(X, y))
                for _ in range(WARM):
                    fn()
                torch.cuda.synchronize()
                steps[f"{how}_{name}"] = stats(timed(fn, SAMPLES, STEPS))
                del e
        out["cfg2_train_step"] = steps
        if not args.no_averaging:
            from slnlp import ops
            n = int(te.layout(cfg)[1])
            avg, p, count = torch.zeros(n, device="cuda"), torch.randn(n, device="cuda"), torch.zeros(1, device="cuda")
            fn = lambda: ops.average_step(avg, p, count, kind="ema", decay=0.999)
            for _ in range(WARM):
                fn()
            torch.cuda.synchronize()
            alone = stats(timed(fn, 40, 1))
            alone.update(arena_floats=n, bytes_moved=12 * n, hbm_peak_bytes_per_s=HBM_PEAK,
                         fraction_of_hbm_peak=12 * n / (alone["median_us"] * 1e-6) / HBM_PEAK)
            out["average_step_alone"] = alone
            for how in ("eager", "graph"):
                out["cfg2_train_step"][f"{how}_batch_minus_off_us"] = steps[f"{how}_batch"]["median_us"] - steps[f"{how}_off"]["median_us"]
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
