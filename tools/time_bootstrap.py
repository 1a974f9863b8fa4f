"""Cost of the bootstrap of the scores on the device (``slnlp_bootstrap_scores``: ``NeuralNetClassifier.score_interval`` /
``compare``) next to the host path it replaces: numpy gathers plus ``metrics.scores_from_rows`` per replicate.

    python tools/time_bootstrap.py [--out profiles/bootstrap_timing.json]

Four points: N = 4000 and N = 800 rows (a full corpus' predictions; a test split) over V = 202 classes, with 1000 and 2000
replicates, top-5 accuracy and Q = 3 value columns (``reliability_rows``' conf, brier, nll).  Per point, on one stream of one
process, into buffers allocated once (``ops.score_interval_buffers``), after 3 warm-up rounds, 12 rounds of: ``ops.score_rows``,
``ops.reliability_rows``, ``ops.bootstrap_scores`` on what they left, the three in a row (``ops.score_interval_rows``: what
``score_interval`` launches) -- each between two HIP events, the second one waited for, the four in an order that rotates from round
to round -- and then the one download (``ops.score_interval_download``), by the wall clock.  The medians are reported.  The host
path, by the wall clock, on the downloaded per-row results: per replicate ``numpy.random`` row indices, the gathers, three
``bincount`` s, ``metrics.scores_from_rows`` for the nine count-derived scores and the column means (no Threefry restatement: the
cheapest honest host bootstrap).  The log-probs are log-softmax of ``3 randn`` logits with the true class raised in 70 % of the
rows.  No pass / fail: the numbers are recorded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

POINTS = ((4000, 202, 1000), (4000, 202, 2000), (800, 202, 1000), (800, 202, 2000))
SAMPLES, WARMUP, HOST_SAMPLES = 12, 3, 3
TOP_K, SEED = 5, 1


def stats(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "min_us": float(v.min()), "max_us": float(v.max())}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e6, out


def make_logp(N, V, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, V, (N,), generator=g)
    logits = 3.0 * torch.randn(N, V, generator=g, dtype=torch.float64)
    rows = torch.nonzero(torch.rand(N, generator=g) < 0.7).squeeze(1)
    logits[rows, y[rows]] += 12.0
    return torch.log_softmax(logits, dim=1).float().cuda(), y.cuda()


def host_bootstrap(y, pred, rank, values, V, B, seed):
    """The host path: stats [B, 9 + Q] from numpy gathers and the project's host scoring."""
    from slnlp import metrics
    names = [*metrics.BOOT_COLUMNS[:8], f"top{TOP_K}_accuracy"]
    rs = np.random.RandomState(seed)
    N = len(y)
    out = np.empty((B, len(names) + values.shape[1]))
    for b in range(B):
        r = rs.randint(0, N, size=N)
        yb, pb = y[r], pred[r]
        counts = np.concatenate([np.bincount(yb, minlength=V), np.bincount(pb, minlength=V), np.bincount(yb[pb == yb], minlength=V), [0]])
        got = metrics.scores_from_rows(names, yb, pb, None, rank[r], counts, V)
        out[b, :len(names)] = [got[n] for n in names]
        out[b, len(names):] = values[r].mean(axis=0)
    return out


def time_point(N, V, B):
    from slnlp import metrics, ops
    logp, y = make_logp(N, V, 1)
    buf = ops.score_interval_buffers(N, V, B, "cuda")
    pred, _, rank, _ = buf["score"]
    rows = buf["reliability"][0]
    calls = {"score_rows": lambda: ops.score_rows(logp, y, out=buf["score"]),
             "reliability_rows": lambda: ops.reliability_rows(logp, y, out=buf["reliability"]),
             "bootstrap_scores": lambda: ops.bootstrap_scores(y, pred, rank, rows[:, :3], n_classes=V, top_k=TOP_K, replicates=B, seed=SEED,
                                                              out=buf["boot"]),
             "score_interval_rows": lambda: ops.score_interval_rows(logp, y, buf, top_k=TOP_K, seed=SEED)}
    names = list(calls)
    us = {k: [] for k in [*names, "download"]}
    for r in range(WARMUP + SAMPLES):
        for name in names[r % len(names):] + names[:r % len(names)]:             # a rotating order
            t = timed(calls[name])
            if r >= WARMUP:
                us[name].append(t)
        t, got = wall(lambda: ops.score_interval_download(buf))
        if r >= WARMUP:
            us["download"].append(t)
    y_host, values = y.cpu().numpy(), rows.cpu().numpy()[:, :3]
    host_us = []
    for r in range(HOST_SAMPLES):
        t0 = time.perf_counter()
        host = host_bootstrap(y_host, got["pred"].astype(np.int64), got["rank"].astype(np.int64), values, V, B, SEED + r)
        host_us.append((time.perf_counter() - t0) * 1e6)
    # two bootstraps of one sample under different generators: their means agree to a few standard errors of a mean
    dev, se = got["stats"], got["stats"].std(axis=0, ddof=1) / np.sqrt(B)
    agree = bool((np.abs(dev.mean(axis=0) - host.mean(axis=0)) <= 6 * np.sqrt(2) * se + 1e-12).all())
    res = {"N": N, "V": V, "replicates": B, "top_k": TOP_K, "value_columns": 3, **{k: stats(v) for k, v in us.items()},
           "host_numpy_per_replicate": stats(host_us), "device_and_host_means_agree": agree,
           "accuracy_interval_device": metrics.bootstrap_intervals(dev[:, :1], ["accuracy"])["accuracy"]}
    res["host_over_device"] = res["host_numpy_per_replicate"]["median_us"] / (res["score_interval_rows"]["median_us"] + res["download"]["median_us"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_bootstrap.py: no GPU -- nothing is measured without one")
    res = {"command": "python tools/time_bootstrap.py --out profiles/bootstrap_timing.json", "device": torch.cuda.get_device_name(0),
           "samples": SAMPLES, "warmup": WARMUP, "host_samples": HOST_SAMPLES, "points": [time_point(*p) for p in POINTS],
           "note": "score_rows, reliability_rows, bootstrap_scores, score_interval_rows: HIP events around one call, the second event waited "
                   "for, in an order that rotates from round to round (score_rows and reliability_rows are two launches each, "
                   "bootstrap_scores is one: a block per replicate; score_interval_rows is the five in a row).  download: wall clock of the "
                   "one device-to-host copy of the replicates, the reliability table and score_rows' results.  host_numpy_per_replicate: "
                   "wall clock of the same number of replicates on the host, from the downloaded per-row results: numpy.random indices, "
                   "gathers, bincounts, metrics.scores_from_rows, column means.  host_over_device = that over score_interval_rows + download"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
