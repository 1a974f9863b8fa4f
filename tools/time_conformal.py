"""Cost of conformal prediction sets on the device (``slnlp_conformal_rows`` / ``_quantile`` / ``_summary``:
``NeuralNetClassifier.conformalize`` / ``predict_set`` / ``coverage``) at the grid's epoch, 4000 rows x 202 classes, next to the
only route to the same numbers without the kernels: download the [N, V] matrix, then the numpy restatement of the same
definitions (tests/conformal_ref.py: one lexsort and one cumsum over the matrix).

    python tools/time_conformal.py [--out profiles/conformal_timing.json]

Measurements, in one process on one stream (randomised APS, alpha 0.1):

* ``kernel``: each launch alone between two HIP events, the second one waited for, into buffers allocated once -- ``rows_scores``
  (labels, no threshold: what calibration runs), ``rows_sets`` (threshold, set words, labels), ``quantile``, ``summary`` (its two
  launches) and ``all_three`` (scores, quantile, sets at the device threshold, summary); 5 warm-up calls, 50 samples each; and
  ``kernel_batched``: 50 calls between one pair of events, divided by 50 (the launch overhead a lone call pays is spread);
* ``device_route``: wall clock of calibrate + predict + report -- the launches, ONE download of the state and the table,
  ``metrics.conformal_report`` -- between two device synchronisations; ``device_route_with_sets`` adds the download of the rows
  and the set words;
* ``host_route``: wall clock of ``logp.cpu()`` and the restatement of the same three steps; it alternates with ``device_route``,
  repeat by repeat (3 warm-up, 10 samples); the two routes' numbers are compared;
* ``end_epoch``: tools/time_epoch_scoring.py's method -- wall clock of ``_FitRun.end_epoch`` of one fit (3200 train / 800 valid
  rows, 202 classes) scoring the reference's five names, with the ``conformal`` option off and on, alternating (5 warm-up, 30
  samples).  The option acts once, at the end of a fit: ``end_epoch`` holds no code of it, so the difference is noise.

The log-probs are log-softmax of ``3 randn`` logits with the true class raised by 1.  No pass / fail: the numbers are recorded."""
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

N, V, ALPHA = 4000, 202, 0.1
CFG = dict(method="aps", randomized=True, seed=1)
KERNEL_WARMUP, KERNEL_SAMPLES, ROUTE_WARMUP, ROUTE_SAMPLES = 5, 50, 3, 10
FIVE = ["neg_log_loss", "accuracy", "precision_weighted", "recall_weighted", "f1_weighted"]


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


def device_route(logp, y, buf, with_sets=False):
    from slnlp import metrics, ops
    ops.conformal_rows(logp, y, buf, draw=0, **CFG)
    ops.conformal_quantile(buf, ALPHA)
    ops.conformal_rows(logp, y, buf, draw=1, qhat=buf["state"], **CFG)
    ops.conformal_summary(buf, y)
    got = ops.conformal_download(buf, rows=with_sets, sets=with_sets)
    return metrics.conformal_report(got["table"], got["state"])


def host_route(logp, y_host):
    import conformal_ref as cr
    from slnlp import metrics
    z = logp.cpu().numpy()
    cal = cr.rows_ref(z, y_host, draw=0, **CFG)
    qhat, n, k, excluded = cr.quantile_ref(cal["score"], cal["rows"][:, 3], ALPHA)
    test = cr.rows_ref(z, y_host, qhat=qhat, draw=1, **CFG)
    cr.pack_sets(test["mask"])
    return metrics.conformal_report(cr.summary_ref(test["rows"], y_host, V), [qhat, n, k, excluded])


def time_kernel_and_routes():
    from slnlp import ops
    logp, y = make_logp(1)
    y_host = y.cpu().numpy()
    buf = ops.conformal_buffers(N, V, "cuda")
    ops.conformal_rows(logp, y, buf, draw=0, **CFG)
    ops.conformal_quantile(buf, ALPHA)
    torch.cuda.synchronize()

    def all_three():
        ops.conformal_rows(logp, y, buf, draw=0, **CFG)
        ops.conformal_quantile(buf, ALPHA)
        ops.conformal_rows(logp, y, buf, draw=1, qhat=buf["state"], **CFG)
        ops.conformal_summary(buf, y)
    calls = {"rows_scores": lambda: ops.conformal_rows(logp, y, buf, draw=0, **CFG),
             "rows_sets": lambda: ops.conformal_rows(logp, y, buf, draw=1, qhat=buf["state"], **CFG),
             "quantile": lambda: ops.conformal_quantile(buf, ALPHA), "summary": lambda: ops.conformal_summary(buf, y), "all_three": all_three}
    kernel, batched = {}, {}
    for name, fn in calls.items():
        kernel[name] = stats([timed_us(fn) for _ in range(KERNEL_WARMUP + KERNEL_SAMPLES)][KERNEL_WARMUP:], "us")
        batched[name] = stats([timed_us(fn, KERNEL_SAMPLES) for _ in range(3 + 10)][3:], "us")
    routes = {"device_route": lambda: device_route(logp, y, buf), "device_route_with_sets": lambda: device_route(logp, y, buf, True),
              "host_route": lambda: host_route(logp, y_host)}
    ms, last = {k: [] for k in routes}, {}
    for r in range(ROUTE_WARMUP + ROUTE_SAMPLES):
        for name in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
            dt, last[name] = wall_ms(routes[name])
            if r >= ROUTE_WARMUP:
                ms[name].append(dt)
    dev, host = last["device_route"], last["host_route"]
    keys = ("qhat", "coverage", "mean_size", "median_size", "empty_rate", "singleton_rate", "worst_class_coverage")
    res = {"kernel": kernel, "kernel_batched": batched, **{k: stats(v, "ms") for k, v in ms.items()},
           "report": {"device": {k: dev[k] for k in keys}, "host": {k: host[k] for k in keys},
                      "max_abs_difference": max(abs(dev[k] - host[k]) for k in keys)}}
    res["host_over_device"] = res["host_route"]["median_ms"] / res["device_route"]["median_ms"]
    res["host_over_device_with_sets"] = res["host_route"]["median_ms"] / res["device_route_with_sets"]["median_ms"]
    return res


def time_end_epoch():
    import time_epoch_scoring as tes
    from slnlp.data import synthetic_dataset
    from slnlp.net import conformal_options
    ds = synthetic_dataset(N, seq_len=12, src_vocab=64, n_labels=V - 2, seed=6, min_len=3)
    cases = {"option_off": tes.make_runs(ds, 1, FIVE), "option_on": tes.make_runs(ds, 1, FIVE)}
    on = cases["option_on"][0][0].net
    on.set_params(conformal={"alpha": ALPHA})
    on._conf_opts = conformal_options(on.conformal)
    ms = {k: [] for k in cases}
    for r in range(tes.WARMUP + tes.REPEATS):
        order = list(cases) if r % 2 == 0 else list(cases)[::-1]
        for name in order:
            dt, _ = tes.one_epoch_end(*cases[name])
            if r >= tes.WARMUP:
                ms[name].append(dt)
    run = cases["option_off"][0][0]
    res = {"train_rows": len(run.tr), "valid_rows": len(run.va), "classes": int(len(run.net.classes_)), **{k: tes.stats(v) for k, v in ms.items()}}
    res["added_ms"] = res["option_on"]["median_ms"] - res["option_off"]["median_ms"]
    res["added_launches"] = 0                               # end_epoch holds no code of the option: it acts once, at the end of a fit
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_conformal.py: no GPU -- nothing is measured without one")
    res = {"command": "python tools/time_conformal.py --out profiles/conformal_timing.json", "device": torch.cuda.get_device_name(0), "N": N, "V": V,
           "alpha": ALPHA, "options": CFG, **time_kernel_and_routes(), "end_epoch": time_end_epoch(),
           "note": "kernel: HIP events around one call, the second event waited for; kernel_batched: 50 calls between one pair of events, per "
                   "call; device_route / host_route: wall clock between two device synchronisations, alternating, of calibrate + predict + "
                   "report through the three entry points with one download of state and table (with_sets: plus rows and set words), and of "
                   "logp.cpu() + the numpy restatement of the same steps; end_epoch: _FitRun.end_epoch of one fit (train and valid split) "
                   "with the conformal option off and on, alternating: the option adds no launch there"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
