"""Cost of the ranking metrics on the device (``slnlp_ranking_rows``: the ``auc_macro`` / ``ap_macro`` scoring names,
``NeuralNetClassifier.ranking``) at the grid's epoch, 4000 rows x 202 classes, next to the only route to the same two numbers
without the kernel: download the [N, V] matrix, then sklearn's binary ``roc_auc_score`` and ``average_precision_score`` per class.

    python tools/time_ranking.py [--out profiles/ranking_timing.json]

Four measurements, in one process on one stream:

* ``kernel``: one ``ops.ranking_rows`` call between two HIP events, the second one waited for, into buffers allocated once --
  without and with the per-row output; 5 warm-up calls, 50 samples each; and ``kernel_batched``: 50 calls between one pair of
  events, divided by 50 (the launch overhead a lone call pays is spread);
* ``device_route``: wall clock of ``metrics.ranking_summary`` -- the launch, the download of V + 1 rows of four doubles and the
  host arithmetic -- between two device synchronisations;
* ``host_route``: wall clock of ``logp.cpu()`` and 2 x (defined classes) sklearn calls, then the two means; it alternates with
  ``device_route``, repeat by repeat (3 warm-up, 10 samples); the two routes' numbers are compared;
* ``end_epoch``: tools/time_epoch_scoring.py's method -- wall clock of ``_FitRun.end_epoch`` of one fit (3200 train / 800 valid
  rows, 202 classes) scoring the reference's five names, without and with ``auc_macro`` and ``ap_macro``, alternating (5
  warm-up, 30 samples).

The log-probs are log-softmax of ``3 randn`` logits with the true class raised by 1.  No pass / fail: the numbers are recorded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

N, V = 4000, 202
KERNEL_WARMUP, KERNEL_SAMPLES, ROUTE_WARMUP, ROUTE_SAMPLES = 5, 50, 3, 10
FIVE = ["neg_log_loss", "accuracy", "precision_weighted", "recall_weighted", "f1_weighted"]
MACRO = ["auc_macro", "ap_macro"]


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


def make_logp(seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, V, (N,), generator=g)
    logits = 3.0 * torch.randn(N, V, generator=g, dtype=torch.float64)
    logits[torch.arange(N), y] += 1.0
    return torch.log_softmax(logits, dim=1).float().cuda(), y.cuda()


def host_route(logp, y_host):
    from sklearn.metrics import average_precision_score, roc_auc_score
    z = logp.cpu().numpy()
    auc, ap = [], []
    for c in range(z.shape[1]):
        pos = y_host == c
        if 0 < pos.sum() < len(pos):
            auc.append(roc_auc_score(pos, z[:, c]))
            ap.append(average_precision_score(pos, z[:, c]))
    return {"auc_macro": float(np.mean(auc)), "ap_macro": float(np.mean(ap)), "classes_scored": len(auc)}


def time_kernel_and_routes():
    from slnlp import metrics, ops
    logp, y = make_logp(1)
    y_host = y.cpu().numpy()
    torch.cuda.synchronize()
    table_only, with_rows = ops.ranking_buffers(N, V, "cuda", per_row=False), ops.ranking_buffers(N, V, "cuda")
    calls = {"table_only": lambda: ops.ranking_rows(logp, y, out=table_only), "with_rows": lambda: ops.ranking_rows(logp, y, out=with_rows)}
    kernel, batched = {}, {}
    for name, fn in calls.items():
        kernel[name] = stats([timed_us(fn) for _ in range(KERNEL_WARMUP + KERNEL_SAMPLES)][KERNEL_WARMUP:], "us")
        batched[name] = stats([timed_us(fn, KERNEL_SAMPLES) for _ in range(3 + 10)][3:], "us")
    ms = {"device_route": [], "host_route": []}
    routes = {"device_route": lambda: metrics.ranking_summary(logp, y, out=table_only), "host_route": lambda: host_route(logp, y_host)}
    last = {}
    for r in range(ROUTE_WARMUP + ROUTE_SAMPLES):
        for name in (("device_route", "host_route") if r % 2 == 0 else ("host_route", "device_route")):
            dt, last[name] = wall_ms(routes[name])
            if r >= ROUTE_WARMUP:
                ms[name].append(dt)
    dev, host = last["device_route"], last["host_route"]
    res = {"kernel": kernel, "kernel_batched": batched, **{k: stats(v, "ms") for k, v in ms.items()},
           "scores": {"device": {k: dev[k] for k in ("auc_macro", "ap_macro", "classes_scored")}, "host": host,
                      "max_abs_difference": max(abs(dev[k] - host[k]) for k in ("auc_macro", "ap_macro"))}}
    res["host_over_device"] = res["host_route"]["median_ms"] / res["device_route"]["median_ms"]
    return res


def time_end_epoch():
    import time_epoch_scoring as tes
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(N, seq_len=12, src_vocab=64, n_labels=V - 2, seed=6, min_len=3)
    cases = {"five_names": tes.make_runs(ds, 1, FIVE), "five_names_and_two_macro": tes.make_runs(ds, 1, FIVE + MACRO)}
    ms = {k: [] for k in cases}
    last = {}
    for r in range(tes.WARMUP + tes.REPEATS):
        order = list(cases) if r % 2 == 0 else list(cases)[::-1]
        for name in order:
            dt, rows = tes.one_epoch_end(*cases[name])
            last[name] = rows[0]
            if r >= tes.WARMUP:
                ms[name].append(dt)
    run = cases["five_names"][0][0]
    res = {"train_rows": len(run.tr), "valid_rows": len(run.va), "classes": int(len(run.net.classes_)), **{k: tes.stats(v) for k, v in ms.items()},
           "valid_auc_macro": last["five_names_and_two_macro"]["valid_auc_macro"], "valid_ap_macro": last["five_names_and_two_macro"]["valid_ap_macro"]}
    res["added_ms"] = res["five_names_and_two_macro"]["median_ms"] - res["five_names"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_ranking.py: no GPU -- nothing is measured without one")
    res = {"command": "python tools/time_ranking.py --out profiles/ranking_timing.json", "device": torch.cuda.get_device_name(0), "N": N, "V": V,
           **time_kernel_and_routes(), "end_epoch": time_end_epoch(),
           "note": "kernel: HIP events around one ops.ranking_rows call (one launch, V blocks), the second event waited for; kernel_batched: 50 calls "
                   "between one pair of events, per call; device_route / host_route: wall clock between two device synchronisations, alternating, "
                   "of metrics.ranking_summary and of logp.cpu() + per-class sklearn roc_auc_score and average_precision_score; end_epoch: "
                   "_FitRun.end_epoch of one fit (train and valid split) with and without the two macro names, alternating"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
