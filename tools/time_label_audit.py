"""Cost of the label audit on the device (``slnlp_label_audit``: ``LogProbJudge.label_issues``) at the grid's epoch, 4000 rows x 202
classes, and at 16384 x 202, next to the only route to the same numbers without the kernels: download the [N, V] matrix, then the
numpy restatement of the same definitions (tests/label_audit_ref.py) and the same report.  And of ``slnlp_scatter_logp``, which
assembles out-of-fold log-probs (``slnlp.OutOfFold``): 5 folds of 800 rows against one ``slnlp_scale_logp`` of 4000 rows.

    python tools/time_label_audit.py [--out profiles/label_audit_timing.json]

Measurements, in one process on one stream (20 pairs):

* ``kernel``: ``slnlp_label_audit`` alone -- its eight launches -- between two HIP events, the second one waited for, into a buffer
  allocated once; 5 warm-up calls, 50 samples; and ``kernel_batched``: 50 calls between one pair of events, divided by 50 (the
  launch overhead a lone call pays is spread);
* ``joint_stages``: the part of that sequence that is not new -- ``ops.confusion_matrix`` on the audit's own (k, y) and
  ``ops.confusion_pairs`` on the joint, four of the eight launches -- timed the same way on the audit's buffers;
* ``device_route``: wall clock of the audit + ONE download (28 bytes a row and the V x V joint) + ``metrics.label_audit_report``,
  between two device synchronisations;
* ``host_route``: wall clock of ``logp.cpu()`` and the restatement (``audit_ref``) with the same report; it alternates with
  ``device_route``, repeat by repeat (3 warm-up, 10 samples);
* ``scatter``: five ``scatter_logp`` calls of 800 rows each into one [4000, 202] buffer, with a temperature state and without,
  and one ``scale_logp`` of the 4000 rows, each group between two HIP events (5 warm-up, 50 samples).

The log-probs are log-softmax of ``3 randn`` logits with the true class raised by 9 and one label in ten redrawn (so there are
label issues to find).  No pass / fail: the numbers are recorded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

V = 202
SIZES = (4000, 16384)
PAIRS = 20
KERNEL_WARMUP, KERNEL_SAMPLES, ROUTE_WARMUP, ROUTE_SAMPLES = 5, 50, 3, 10
FOLDS, FOLD_ROWS = 5, 800


def stats(v, unit):
    v = np.asarray(v)
    return {f"median_{unit}": float(np.median(v)), f"min_{unit}": float(v.min()), f"max_{unit}": float(v.max())}


def timed_us(fn, calls=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def make_logp(N, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, V, (N,), generator=g)
    logits = 3.0 * torch.randn(N, V, generator=g, dtype=torch.float64)
    logits[torch.arange(N), y] += 9.0
    noisy = torch.where(torch.rand(N, generator=g) < 0.1, torch.randint(0, V, (N,), generator=g), y)
    return torch.log_softmax(logits, dim=1).float().cuda(), noisy.cuda()


def device_route(logp, y, y_host, buf):
    from slnlp import metrics, ops
    ops.label_audit_rows(logp, y, buf)
    return metrics.label_audit_report(ops.label_audit_download(buf), y_host)


def host_route(logp, y_host):
    import label_audit_ref as lr
    from slnlp import metrics
    return metrics.label_audit_report(lr.record_of(lr.audit_ref(logp.cpu().numpy(), y_host, pairs=PAIRS)), y_host)


def time_size(N):
    from slnlp import ops
    logp, y = make_logp(N, 1)
    y_host = y.cpu().numpy()
    buf = ops.label_audit_buffers(N, V, PAIRS, "cuda")
    ops.label_audit_rows(logp, y, buf)
    torch.cuda.synchronize()
    audit = lambda: ops.label_audit_rows(logp, y, buf)
    kernel = stats([timed_us(audit) for _ in range(KERNEL_WARMUP + KERNEL_SAMPLES)][KERNEL_WARMUP:], "us")
    batched = stats([timed_us(audit, KERNEL_SAMPLES) for _ in range(3 + 10)][3:], "us")
    at, flat = buf["at"], buf["flat"]
    k, joint = flat[at["k"]:at["k"] + N], flat[at["joint"]:at["joint"] + V * V + 1]
    top, work = flat[at["pairs"]:at["pairs"] + 3 * PAIRS].view(PAIRS, 3), flat[at["work"]:].view(torch.uint8)

    def joint_stages():
        ops.confusion_matrix(k, y, V, out=joint)
        ops.confusion_pairs(joint, V, PAIRS, out=top, work=work)
    stages = stats([timed_us(joint_stages) for _ in range(KERNEL_WARMUP + KERNEL_SAMPLES)][KERNEL_WARMUP:], "us")
    routes = {"device_route": lambda: device_route(logp, y, y_host, buf), "host_route": lambda: host_route(logp, y_host)}
    ms, last = {k: [] for k in routes}, {}
    for r in range(ROUTE_WARMUP + ROUTE_SAMPLES):
        for name in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
            dt, last[name] = wall_ms(routes[name])
            if r >= ROUTE_WARMUP:
                ms[name].append(dt)
    dev, host = last["device_route"], last["host_route"]
    keys = ("rows", "unconfident", "argmax_disagrees")
    res = {"N": N, "V": V, "pairs": PAIRS, "kernel": kernel, "kernel_batched": batched, "joint_stages": stages,
           **{name: stats(v, "ms") for name, v in ms.items()},
           "report": {"device": {**{k: dev[k] for k in keys}, "issues": int(len(dev["issues"]["row"])), "noise_rate": dev["noise_rate"]},
                      "host": {**{k: host[k] for k in keys}, "issues": int(len(host["issues"]["row"])), "noise_rate": host["noise_rate"]},
                      "issues_equal": bool(np.array_equal(dev["issues"]["row"], host["issues"]["row"])),
                      "joint_equal": bool(np.array_equal(dev["joint"], host["joint"])), "pairs_equal": dev["pairs"] == host["pairs"]}}
    res["host_over_device"] = res["host_route"]["median_ms"] / res["device_route"]["median_ms"]
    return res


def time_scatter():
    from slnlp import ops
    N = FOLDS * FOLD_ROWS
    logp, _ = make_logp(N, 2)
    state = ops.temperature_state(0.8, "cuda")
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3))
    parts = [(logp[f * FOLD_ROWS:(f + 1) * FOLD_ROWS], perm[f * FOLD_ROWS:(f + 1) * FOLD_ROWS].contiguous().cuda()) for f in range(FOLDS)]
    out, scaled = torch.empty(N, V, dtype=torch.float32, device="cuda"), torch.empty(N, V, dtype=torch.float32, device="cuda")

    def scatter(st):
        for z, rows in parts:
            ops.scatter_logp(z, rows, out, state=st)
    calls = {"scatter_5x800_with_state": lambda: scatter(state), "scatter_5x800_copy": lambda: scatter(None),
             "scale_logp_4000": lambda: ops.scale_logp(logp, state, out=scaled)}
    res = {name: stats([timed_us(fn) for _ in range(KERNEL_WARMUP + KERNEL_SAMPLES)][KERNEL_WARMUP:], "us") for name, fn in calls.items()}
    scatter(state)
    ops.scale_logp(logp, state, out=scaled)
    torch.cuda.synchronize()
    res["bits_equal"] = bool(torch.equal(out[perm.cuda()], scaled))
    return {"N": N, "V": V, "folds": FOLDS, **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_label_audit.py: no GPU -- nothing is measured without one")
    res = {"command": "python tools/time_label_audit.py --out profiles/label_audit_timing.json", "device": torch.cuda.get_device_name(0),
           "sizes": [time_size(N) for N in SIZES], "scatter": time_scatter(),
           "note": "kernel: HIP events around one slnlp_label_audit call (eight launches), the second event waited for; kernel_batched: 50 "
                   "calls between one pair of events, per call; joint_stages: the confusion_matrix and confusion_pairs launches of that sequence alone; device_route / host_route: wall clock between two device synchronisations, "
                   "alternating, of the audit + one download + metrics.label_audit_report, and of logp.cpu() + the numpy restatement + the "
                   "same report; scatter: five scatter_logp calls of 800 rows (with a temperature state / plain copy) and one scale_logp of "
                   "4000 rows, HIP events around each group"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
