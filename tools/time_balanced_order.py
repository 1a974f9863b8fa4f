"""Cost of a class-balanced epoch's draw on the device against the host draw it stands in for, and the host round trips of
one epoch with and without it.

    python tools/time_balanced_order.py [--out profiles/balanced_order_timing.json]

* ``slnlp_balanced_order`` at n = 4000 rows in 200 classes (skewed counts): HIP events around each of 200 calls after 20
  warm-up calls, on one stream.
* the host path of a shuffled epoch at the same n: ``EpochOrder.next_epoch()`` + the visit table (range check, labels in visit
  order) + its upload, wall clock with the upload waited for, same call counts.
* one epoch of a small LSTM fit, balanced and shuffled: how often the host waits for the device (``Tensor.cpu`` /
  ``Tensor.item`` / event and stream synchronisation calls made from Python) and how many host-to-device copies it issues.
No pass / fail: the numbers are recorded, the feature is not justified by speed."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

N, CLASSES, CALLS, WARMUP = 4000, 200, 200, 20


def skewed_labels():
    rs = np.random.RandomState(0)
    w = rs.pareto(1.5, CLASSES) + 0.05
    counts = np.maximum(2, np.floor(w / w.sum() * N)).astype(np.int64)
    counts[np.argmax(counts)] += N - counts.sum()
    assert counts.sum() == N and counts.min() >= 2
    return rs.permutation(np.repeat(np.arange(CLASSES), counts)).astype(np.int64), counts


def stats(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "mean_us": float(v.mean()), "min_us": float(v.min()), "max_us": float(v.max())}


def time_device(y):
    from slnlp import ops
    yd = torch.from_numpy(y).cuda()
    plan = ops.BalancePlan(y, CLASSES)
    out = (torch.empty(plan.rows, dtype=torch.int64, device="cuda"), torch.empty(plan.rows, dtype=torch.int64, device="cuda"))
    us = []
    for k in range(WARMUP + CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        plan.order(yd, 12345, k, out=out)
        b.record()
        b.synchronize()
        if k >= WARMUP:
            us.append(a.elapsed_time(b) * 1e3)
    return plan.rows, stats(us)


def time_host(y):
    from slnlp import sampler
    orders = sampler.EpochOrder(N, 50, 12345)
    us = []
    for k in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        order = sampler.check_order(orders.next_epoch(), N, N)
        dev = torch.from_numpy(np.stack([order, y[order]])).to("cuda")
        torch.cuda.synchronize()
        if k >= WARMUP:
            us.append((time.perf_counter() - t0) * 1e6)
    del dev
    return stats(us)


def epoch_round_trips(option):
    """Host waits and uploads of ONE train + valid epoch (the second of a fit: plans built, tables warm)."""
    from slnlp.data import synthetic_dataset
    from slnlp.net import NeuralNetClassifier
    ds = synthetic_dataset(200, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)
    torch.manual_seed(1)
    net = NeuralNetClassifier(module="model.EncoderDecoderLSTMAttn", module__dropout=0.0, module__src_vocab=ds.vocab_X,
                              module__tgt_vocab=ds.vocab_y, module__batch_first=True, module__embedding_size=24, module__hidden_size=32,
                              module__num_layers=2, criterion__ignore_index=1, optimizer__momentum=0.9, lr=0.05, max_epochs=1, batch_size=20,
                              use_graph=False, gradient_clipping={"gradient_clip_value": 0.5}, **{f"iterator_train__{option}": True})
    net.fit(ds)
    counts = {"host_waits": 0, "host_to_device_copies": 0}
    saved = {}

    def wrap(owner, name, key, when=lambda *a, **k: True):
        orig = getattr(owner, name)
        saved[(owner, name)] = orig

        def f(*a, **k):
            if when(*a, **k):
                counts[key] += 1
            return orig(*a, **k)
        setattr(owner, name, f)
    wrap(torch.Tensor, "cpu", "host_waits", lambda t, *a, **k: t.is_cuda)
    wrap(torch.Tensor, "item", "host_waits", lambda t, *a, **k: t.is_cuda)
    wrap(torch.cuda.Event, "synchronize", "host_waits")
    wrap(torch.cuda.Stream, "synchronize", "host_waits")
    wrap(torch.Tensor, "to", "host_to_device_copies", lambda t, *a, **k: not t.is_cuda and "cuda" in str(a) + str(k))
    try:
        net.partial_fit(ds)
    finally:
        for (owner, name), orig in saved.items():
            setattr(owner, name, orig)
    counts["train_batches"] = sum("train_loss" in b for b in net.history[-1]["batches"])
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    y, counts = skewed_labels()
    rows, dev = time_device(y)
    res = {"command": "python tools/time_balanced_order.py --out profiles/balanced_order_timing.json",
           "device": torch.cuda.get_device_name(0), "n": N, "classes": CLASSES, "largest_class": int(counts.max()), "n_bal": rows,
           "calls": CALLS, "warmup": WARMUP,
           "slnlp_balanced_order_hip_events": dev,
           "host_draw_table_upload_wall_clock": time_host(y),
           "one_epoch_round_trips": {"balanced": epoch_round_trips("balance"), "shuffled": epoch_round_trips("shuffle")},
           "note": "host_waits: Tensor.cpu / Tensor.item on device tensors, Event.synchronize, Stream.synchronize called from Python "
                   "during the second epoch of a 200-row LSTM fit (train + valid pass, no scoring metrics)"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
