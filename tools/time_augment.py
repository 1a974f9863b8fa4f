"""Cost of a train epoch's augmentation draw on the device (``iterator_train__augment``, ``slnlp_augment_rows``) against its
floor, a plain device copy of the same two buffers.

    python tools/time_augment.py [--out profiles/augment_timing.json]

Two shapes: the reference's train split (4000 rows of 48 positions) and one batch-sized toy (50 x 12, which measures the launch).
Per shape the draw and the copy (``X_out.copy_(X)``, ``L_out.copy_(L)``: two torch copy launches over the same bytes) alternate
in one process on one stream: HIP events around each of 200 calls of either after 20 warm-up calls of both, and around 20
back-to-back windows of 50 calls (a single call is a few microseconds, the events' own resolution).  The epoch number moves
from call to call, as it does in a fit.  No pass / fail: the numbers are recorded, the feature is not justified by speed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

SHAPES = ((4000, 48), (50, 12))
CALLS, WARMUP, WINDOWS, PER_WINDOW = 200, 20, 20, 50
P_DROP, P_MASK, PAD, UNK, SEED = 0.1, 0.1, 1, 0, 12345


def stats(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "mean_us": float(v.mean()), "min_us": float(v.min()), "max_us": float(v.max())}


def timed(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def time_shape(n, S):
    from slnlp import ops
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(n, seq_len=S, src_vocab=3000, n_labels=200, seed=1, min_len=min(8, S))
    X, L = torch.from_numpy(ds.ids).cuda(), torch.from_numpy(ds.lengths).cuda()
    out = (torch.empty_like(X), torch.empty_like(L))

    def draw(k):
        ops.augment_rows(X, L, PAD, UNK, P_DROP, P_MASK, SEED, k, out=out)

    def copy(k):
        out[0].copy_(X)
        out[1].copy_(L)

    def window(fn):
        def run(k):
            for j in range(PER_WINDOW):
                fn(k * PER_WINDOW + j)
        return run
    single = {"draw": [], "copy": []}
    for k in range(WARMUP + CALLS):
        for name, fn in (("draw", draw), ("copy", copy)):
            us = timed(fn, k)
            if k >= WARMUP:
                single[name].append(us)
    back_to_back = {"draw": [], "copy": []}
    for k in range(WINDOWS):
        for name, fn in (("draw", draw), ("copy", copy)):
            back_to_back[name].append(timed(window(fn), k) / PER_WINDOW)
    draw(0)
    kept = float(out[1].sum().item()) / float(L.sum().item())
    return {"n": n, "S": S, "bytes_read_and_written": int(2 * (X.numel() + L.numel()) * 8),
            "positions_kept_fraction_epoch0": kept,
            "one_call_between_events": {"slnlp_augment_rows": stats(single["draw"]), "device_copy_of_both_buffers": stats(single["copy"])},
            "per_call_in_windows_of_%d" % PER_WINDOW: {"slnlp_augment_rows": stats(back_to_back["draw"]),
                                                       "device_copy_of_both_buffers": stats(back_to_back["copy"])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_augment.py: no GPU -- nothing is measured without one")
    res = {"command": "python tools/time_augment.py --out profiles/augment_timing.json", "device": torch.cuda.get_device_name(0),
           "p_drop": P_DROP, "p_mask": P_MASK, "calls": CALLS, "warmup": WARMUP, "windows": WINDOWS,
           "shapes": [time_shape(n, S) for n, S in SHAPES],
           "note": "draw and copy alternate call by call (and window by window) on one stream; the copy is two torch launches "
                   "(ids, lengths), the draw one launch"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
