"""Cost of selective prediction on the device (``slnlp_selective_rows`` / ``_counts``: ``NeuralNetClassifier.risk_coverage`` /
``fit_rejection`` / ``predict_selective``) at the grid's epoch, 4000 rows x 202 classes, and at 16384 x 202 (eight chunks of
included rows), next to the only route to the same numbers without the kernels: download the [N, V] matrix, then the numpy
restatement of the same definitions (tests/selective_ref.py: one pass over the matrix, two sorts and two searches over the rows).

    python tools/time_selective.py [--out profiles/selective_timing.json]

Measurements, in one process on one stream (score max_prob unless named; three risk and four coverage levels):

* ``kernel``: each call alone between two HIP events, the second one waited for, into buffers allocated once -- ``rows_max_prob``,
  ``rows_margin``, ``rows_neg_entropy``, ``counts`` (its three launches) and ``rows_and_counts``; 5 warm-up calls, 50 samples each;
  and ``kernel_batched``: 50 calls between one pair of events, divided by 50 (the launch overhead a lone call pays is spread);
* ``device_route``: wall clock of rows + counts + ONE download (32 bytes a row) + ``metrics.selective_report`` with the curve,
  between two device synchronisations;
* ``host_route``: wall clock of ``logp.cpu()`` and the restatement of the same steps (``rows_ref``, ``table_ref``) and the same
  report; it alternates with ``device_route``, repeat by repeat (3 warm-up, 10 samples);
* ``host_counts``: wall clock of the restatement's counts alone (``counts_ref``: numpy's two sorts and two searches on a kappa
  that is already on the host): what the counts kernel, whose work grows with N^2 / 2048, competes with once the rows are reduced.

The log-probs are log-softmax of ``3 randn`` logits with the true class raised by 9 (about half of the arg-maxes are right, so every
level has an answer).  No pass / fail: the numbers are recorded."""
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
RISKS, COVERAGES = [0.01, 0.05, 0.1], [0.5, 0.8, 0.9, 1.0]
SCORES = ("max_prob", "margin", "neg_entropy")
KERNEL_WARMUP, KERNEL_SAMPLES, ROUTE_WARMUP, ROUTE_SAMPLES = 5, 50, 3, 10


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


def wall_ms(fn, sync=True):
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def make_logp(N, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, V, (N,), generator=g)
    logits = 3.0 * torch.randn(N, V, generator=g, dtype=torch.float64)
    logits[torch.arange(N), y] += 9.0
    return torch.log_softmax(logits, dim=1).float().cuda(), y.cuda()


def device_route(logp, y, buf):
    from slnlp import metrics, ops
    ops.selective_rows(logp, y, buf)
    ops.selective_counts(buf, RISKS, COVERAGES)
    got = ops.selective_download(buf)
    return metrics.selective_report(got["kappa"], got["rows"], got["counts"], got["table"], RISKS, COVERAGES)


def host_route(logp, y_host):
    import selective_ref as sr
    from slnlp import metrics
    z = logp.cpu().numpy()
    rows = sr.rows_ref(z, y_host)
    table, s = sr.table_ref(rows["kappa"], rows["rows"], RISKS, COVERAGES)
    return metrics.selective_report(rows["kappa"], rows["rows"], s["counts"], table, RISKS, COVERAGES)


def time_size(N):
    import selective_ref as sr
    from slnlp import ops
    logp, y = make_logp(N, 1)
    y_host = y.cpu().numpy()
    buf = ops.selective_buffers(N, "cuda")
    ops.selective_rows(logp, y, buf)
    ops.selective_counts(buf, RISKS, COVERAGES)
    torch.cuda.synchronize()

    def both():
        ops.selective_rows(logp, y, buf)
        ops.selective_counts(buf, RISKS, COVERAGES)
    calls = {**{f"rows_{s}": (lambda s=s: ops.selective_rows(logp, y, buf, score=s)) for s in SCORES[::-1]},      # max_prob last: counts reads it
             "counts": lambda: ops.selective_counts(buf, RISKS, COVERAGES), "rows_and_counts": both}
    kernel, batched = {}, {}
    for name, fn in calls.items():
        kernel[name] = stats([timed_us(fn) for _ in range(KERNEL_WARMUP + KERNEL_SAMPLES)][KERNEL_WARMUP:], "us")
        batched[name] = stats([timed_us(fn, KERNEL_SAMPLES) for _ in range(3 + 10)][3:], "us")
    routes = {"device_route": lambda: device_route(logp, y, buf), "host_route": lambda: host_route(logp, y_host)}
    ms, last = {k: [] for k in routes}, {}
    for r in range(ROUTE_WARMUP + ROUTE_SAMPLES):
        for name in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
            dt, last[name] = wall_ms(routes[name])
            if r >= ROUTE_WARMUP:
                ms[name].append(dt)
    got = ops.selective_download(buf)
    host_counts = [wall_ms(lambda: sr.counts_ref(got["kappa"], got["rows"]), sync=False)[0] for _ in range(3 + 10)][3:]
    dev, host = last["device_route"], last["host_route"]
    keys = ("rows", "errors", "aurc", "aurc_oracle", "e_aurc")
    levels = lambda rep: [(e["accepted"], e["wrong"]) for e in rep["coverage_at_risk"] + rep["risk_at_coverage"]]
    res = {"N": N, "V": V, "chunks": (N + 2047) // 2048, "kernel": kernel, "kernel_batched": batched, **{k: stats(v, "ms") for k, v in ms.items()},
           "host_counts": stats(host_counts, "ms"),
           "report": {"device": {k: dev[k] for k in keys}, "host": {k: host[k] for k in keys},
                      "levels": levels(dev), "levels_equal": levels(dev) == levels(host),
                      "max_abs_difference": max(abs(dev[k] - host[k]) for k in keys)}}
    res["host_over_device"] = res["host_route"]["median_ms"] / res["device_route"]["median_ms"]
    res["counts_kernel_over_host_counts"] = kernel["counts"]["median_us"] * 1e-3 / res["host_counts"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_selective.py: no GPU -- nothing is measured without one")
    res = {"command": "python tools/time_selective.py --out profiles/selective_timing.json", "device": torch.cuda.get_device_name(0),
           "risks": RISKS, "coverages": COVERAGES, "sizes": [time_size(N) for N in SIZES],
           "note": "kernel: HIP events around one call, the second event waited for; kernel_batched: 50 calls between one pair of events, per "
                   "call; device_route / host_route: wall clock between two device synchronisations, alternating, of rows + counts + one "
                   "download + metrics.selective_report, and of logp.cpu() + the numpy restatement + the same report; host_counts: the "
                   "restatement's counts alone (numpy sorts and searches) on a host kappa; counts_kernel_over_host_counts above 1 means the counts kernel "
                   "is slower than the host at that N"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
