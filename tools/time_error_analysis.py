"""Cost of the error analysis on the device (``slnlp_topk_rows``, ``slnlp_confusion_matrix``, ``slnlp_confusion_pairs``:
``NeuralNetClassifier.predict_topk`` / ``error_analysis``) next to the host path it replaces: downloading the [N, V] log-probs and
reducing them with numpy.

    python tools/time_error_analysis.py [--out profiles/error_analysis_timing.json]

Two shapes: N = 4000 with V = 202 (the goldens' target classes) and with V = 2048 (the full corpus' order of magnitude).  Per shape,
on one stream of one process, into buffers allocated once (``ops.error_analysis_buffers``), after 3 warm-up rounds, 12 rounds of:
``ops.topk_rows`` (k = 5, beta = 1 as the null pointer), ``ops.confusion_matrix`` on ``score_rows``' predictions, ``ops.confusion_pairs``
(M = 20) and the three in a row with ``score_rows`` in front (``ops.error_analysis_rows``: what ``error_analysis`` launches) --
each between two HIP events, the second one waited for -- and then the one download of the pairs, the class counts and the top-k
lists, by the wall clock.  The host path, by the wall clock: ``logp.cpu()`` and then tests/confusion_ref.py's numpy restatement
of the same three results (per-row ``lexsort``, ``add.at``, a stable sort of the cells).  The log-probs are log-softmax of
``3 randn`` logits with the true class raised in half of the rows.  No pass / fail: the numbers are recorded."""
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

SHAPES = ((4000, 202), (4000, 2048))
SAMPLES, WARMUP = 12, 3
K, M = 5, 20


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
    rows = torch.nonzero(torch.rand(N, generator=g) < 0.5).squeeze(1)
    logits[rows, y[rows]] += 12.0
    return torch.log_softmax(logits, dim=1).float().cuda(), y.cuda()


def time_shape(N, V):
    from confusion_ref import confusion_ref, pairs_ref, topk_ref
    from slnlp import ops
    logp, y = make_logp(N, V, 1)
    buf = ops.error_analysis_buffers(N, V, K, M, "cuda")
    ops.score_rows(logp, y, out=buf["score"])
    calls = {"topk_rows": lambda: ops.topk_rows(logp, K, out=buf["topk"]),
             "confusion_matrix": lambda: ops.confusion_matrix(buf["pred"], y, V, out=buf["confusion"]),
             "confusion_pairs": lambda: ops.confusion_pairs(buf["confusion"], V, M, out=buf["pairs"], work=buf["work"]),
             "error_analysis_rows": lambda: ops.error_analysis_rows(logp, y, buf)}
    us = {k: [] for k in calls}
    us["download"] = []
    for r in range(WARMUP + SAMPLES):
        for name, fn in calls.items():
            t = timed(fn)
            if r >= WARMUP:
                us[name].append(t)
        t, got = wall(lambda: ops.error_analysis_download(buf, matrix=False, topk=True))
        if r >= WARMUP:
            us["download"].append(t)

    def host():
        z = logp.cpu().numpy()
        idx, prob = topk_ref(z, K)
        counts = confusion_ref(z.argmax(axis=1), y_host, V)
        return idx, prob, pairs_ref(counts, V, M)
    y_host = y.cpu().numpy()
    host_us = []
    for r in range(3):
        t, (idx, prob, pairs) = wall(host)
        host_us.append(t)
    same = bool(np.array_equal(got["topk_idx"], idx) and np.array_equal(got["pairs"], pairs)
                and np.abs(got["topk_prob"] - prob).max() <= 1e-9)
    res = {"N": N, "V": V, "k": K, "pairs": M, **{k: stats(v) for k, v in us.items()}, "host_download_and_numpy": stats(host_us),
           "device_equals_host": same}
    res["host_over_device"] = res["host_download_and_numpy"]["median_us"] / (res["error_analysis_rows"]["median_us"] + res["download"]["median_us"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_error_analysis.py: no GPU -- nothing is measured without one")
    res = {"command": "python tools/time_error_analysis.py --out profiles/error_analysis_timing.json", "device": torch.cuda.get_device_name(0),
           "samples": SAMPLES, "warmup": WARMUP, "host_samples": 3, "shapes": [time_shape(N, V) for N, V in SHAPES],
           "note": "topk_rows, confusion_matrix, confusion_pairs, error_analysis_rows: HIP events around one call, the second event waited "
                   "for (topk_rows is one launch, confusion_matrix two -- zeroing the counts, then the rows --, confusion_pairs two -- the "
                   "slices, then the merge; error_analysis_rows is score_rows' two launches and these five).  download: wall clock of the "
                   "one device-to-host copy of pairs, class counts and top-k lists (matrix=False).  host_download_and_numpy: wall clock of "
                   "logp.cpu() and the numpy restatement of the same three results (tests/confusion_ref.py).  host_over_device = that over "
                   "error_analysis_rows + download"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
