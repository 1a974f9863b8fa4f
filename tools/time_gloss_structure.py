"""Cost of the gloss structure pass (``slnlp_gloss_structure_begin`` / ``_rows`` / ``_finish``, csrc/gloss_structure.hip:
``slnlp.gloss_structure``) next to the distance launch that feeds it and next to the host route to the same integers.

    python tools/time_gloss_structure.py [--out profiles/gloss_structure_timing.json]

Rows of 48 positions from ``synthetic_dataset`` (3000 source tokens, lengths 8..48) with 202 classes, at 4000 and at 16384 rows; the
unit-cost metric.  Everything runs on a stream of its own with nothing else on the GPU.  Event-timed as tools/time_dup_groups.py:
the calls between two HIP events, the second one waited for, into buffers allocated once; 5 warm-up calls, 30 samples;
``*_batched``: 10 calls between one pair of events, divided by 10.  No pass / fail: the numbers are recorded.

* ``edit_distances``: the distance launch alone, all N x N pairs (one chunk at both sizes: 16384^2 bytes are the 256 MiB scratch).
* ``rows``: ``ops.gloss_structure_rows`` alone over that matrix.  It adds into class_sum and takes minima into med_sum, so each
  sample is begin + rows, and ``begin`` alone (its two launches) is recorded beside it to be taken off.
* ``sequence``: begin, distances, rows, finish -- what ``gloss_structure`` queues, without the uploads and the download.
* ``gloss_structure``: the public call, wall clock between two device synchronisations, with its uploads, its one download and the
  host report (3 warm-up, 10 samples).
* ``host_route``: the same integers by the host in the same run: the distance launch, the matrix downloaded, numpy (the columns
  sorted by class, ``np.add.reduceat`` into per-row class sums, the exact argmin by cross-multiplication class by class); wall
  clock, 3 samples; ``same_integers``: whether own, other, other_class, class_sum and the medoids equal the device's."""
import argparse
import json
import os
import sys
import time

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "sign-language-nlp_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

S, SRC_VOCAB, CLASSES, BOUND = 48, 3000, 202, 64
SIZES = (4000, 16384)
WARMUP, SAMPLES, BATCH = 5, 30, 10


def stats(v, unit):
    v = np.asarray(v)
    return {f"median_{unit}": float(np.median(v)), f"min_{unit}": float(v.min()), f"max_{unit}": float(v.max())}


def timed_us(fn, calls=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def sampled(fn):
    lone = stats([timed_us(fn) for _ in range(WARMUP + SAMPLES)][WARMUP:], "us")
    batched = stats([timed_us(fn, BATCH) for _ in range(3 + 10)][3:], "us")
    return lone, batched


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_structure(dist, label, C):
    """own, other, other_class, class_sum, medoid of a square uint8 matrix whose rows are all labelled (0..C-1), in numpy"""
    N = len(label)
    order = np.argsort(label, kind="stable")
    count = np.bincount(label, minlength=C).astype(np.int64)
    present = np.flatnonzero(count)
    starts = np.concatenate([[0], np.cumsum(count[present])[:-1]])
    T = np.zeros((N, C), dtype=np.int64)
    T[:, present] = np.add.reduceat(dist[:, order], starts, axis=1, dtype=np.int64)        # the diagonal holds 0: d(i, i) adds nothing
    rows = np.arange(N)
    own = T[rows, label]
    best = np.full(N, -1, dtype=np.int64)
    for c in present:
        free = (label != c)
        first = free & (best < 0)
        safe = np.where(best < 0, 0, best)
        better = free & (best >= 0) & (T[:, c] * count[safe] < T[rows, safe] * count[c])
        best[first | better] = c
    other = np.where(best >= 0, T[rows, np.where(best < 0, 0, best)], 0)
    class_sum = np.zeros((C, C), dtype=np.int64)
    np.add.at(class_sum, label, T)
    key = own * N + rows                                     # the smallest own, then the lowest row
    low = np.full(C, np.iinfo(np.int64).max)
    np.minimum.at(low, label, key)
    medoid = np.where(count > 0, low % N, -1)
    return own, other, best, class_sum, medoid


def time_size(n):
    import torch
    import slnlp
    from slnlp import _lib, ops
    from slnlp.data import synthetic_dataset
    print(f"[time_gloss_structure] {n} rows ...", file=sys.stderr, flush=True)
    ds = synthetic_dataset(n, seq_len=S, src_vocab=SRC_VOCAB, n_labels=CLASSES, seed=1, min_len=8)
    classes, label = np.unique(np.asarray(ds.y), return_inverse=True)
    label = label.reshape(-1).astype(np.int64)
    C = len(classes)
    res = {"rows": n, "S": S, "classes": C, "pairs": n * n, "matrix_bytes": n * n}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        X, L = torch.from_numpy(ds.ids).cuda(), torch.from_numpy(ds.lengths).cuda()
        dist = torch.empty(n, n, dtype=torch.uint8, device="cuda")
        buf = ops.gloss_structure_buffers(n, C, label, BOUND, "cuda")
        begin = lambda: _lib.check(_lib.load().slnlp_gloss_structure_begin(
            buf["label"].data_ptr(), n, C, BOUND, buf["count"].data_ptr(), buf["class_sum"].data_ptr(), buf["med_sum"].data_ptr(),
            buf["medoid"].data_ptr(), buf["head"].data_ptr(), _lib.stream_ptr()), "gloss_structure_begin")
        distances = lambda: ops.edit_distances(X, L, X, L, out=dist)
        rows = lambda: ops.gloss_structure_rows(dist, 0, buf)

        def sequence():
            begin(); distances(); rows(); ops.gloss_structure_finish(buf)
        res["edit_distances"], res["edit_distances_batched"] = sampled(distances)
        res["begin"], res["begin_batched"] = sampled(begin)
        res["begin_rows"], res["begin_rows_batched"] = sampled(lambda: (begin(), rows()))
        res["rows_batched_median_us"] = res["begin_rows_batched"]["median_us"] - res["begin_batched"]["median_us"]
        res["rows_median_us"] = res["begin_rows"]["median_us"] - res["begin"]["median_us"]
        res["sequence"], res["sequence_batched"] = sampled(sequence)
        sequence()
        device = {k: v.copy() for k, v in ops.gloss_structure_download(buf).items()}
        res["rows_over_distances"] = res["rows_batched_median_us"] / res["edit_distances_batched"]["median_us"]
        stream.synchronize()

        def host_route():
            distances()
            return host_structure(dist.cpu().numpy(), label, C)
        took = [wall_ms(host_route) for _ in range(3)]
        res["host_route"] = stats([t for t, _ in took], "ms")
        own, other, best, class_sum, medoid = took[-1][1]
        res["same_integers"] = bool(np.array_equal(own, device["own"]) and np.array_equal(other, device["other"])
                                    and np.array_equal(best, device["other_class"]) and np.array_equal(class_sum, device["class_sum"])
                                    and np.array_equal(medoid, device["medoid"]))

        def download_only():
            distances()
            return dist.cpu().numpy()
        res["host_route_download"] = stats([wall_ms(download_only)[0] for _ in range(3)], "ms")
    public = [wall_ms(lambda: slnlp.gloss_structure(ds)) for _ in range(3 + 10)][3:]
    res["gloss_structure"] = stats([t for t, _ in public], "ms")
    rep = public[-1][1]
    res["same_medoids_public"] = bool(np.array_equal(rep["medoids"], device["medoid"]))
    res["mean_silhouette"], res["misplaced_share"] = rep["mean_silhouette"], rep["misplaced_share"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_gloss_structure.py: no GPU -- nothing is measured without one")
    res = {"command": "python tools/time_gloss_structure.py --out profiles/gloss_structure_timing.json", "device": torch.cuda.get_device_name(0),
           "sizes": [time_size(n) for n in SIZES],
           "note": (f"HIP events around the calls on a stream of its own, the second event waited for, {SAMPLES} samples after {WARMUP} warm-up; "
                    f"*_batched: {BATCH} calls between one pair of events, per call; rows = (begin + rows) - begin, medians; "
                    "gloss_structure and host_route: wall clock between two device synchronisations; the rows are synthetic and their "
                    "labels random: the silhouette recorded here says nothing about real data")}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
