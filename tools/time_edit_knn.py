"""Cost of the edit-distance neighbour search on the device (``slnlp_edit_distances`` / ``slnlp_edit_knn_rows`` /
``slnlp_edit_knn_logp``: ``slnlp.EditKNN``, ``slnlp.split_audit``).

    python tools/time_edit_knn.py [--out profiles/edit_knn_timing.json] [--host-queries 8]
    python tools/time_edit_knn.py --ab parent [--out profiles/knn_shell_timing.json]

Rows of S = 48 positions from ``synthetic_dataset`` (3000 source tokens, 200 labels, lengths 8..48), k = 5, at three shapes (queries
x references): 800 x 3200 (a grid's test split against its train split), 4000 x 4000 (leave-one-out over a train split) and
16384 x 4000 (where its one byte per pair of scratch fits).  In one process on one stream, per shape:

* ``distances``, ``knn_rows``, ``knn_logp``: one ``ops`` call each -- one, three and two launches -- between two HIP events, the
  second one waited for, into buffers allocated once; 5 warm-up calls, 30 samples; ``*_batched``: 10 calls between one pair of
  events, divided by 10 (the launch overhead a lone call pays is spread).  ``pairs_per_us``: pairs over the distance kernel's
  batched median -- a rate of whole dynamic programs, not a share of any peak;
* ``predict_proba``: wall clock, between two device synchronisations, of ``EditKNN.predict_proba`` on the query rows -- upload,
  the five launches, its one download of [nq, V] float32 and the host softmax (3 warm-up, 10 samples);
* ``host``: the numpy / python restatement (tests/edit_knn_ref.py: distances, selection, vote) on the FIRST ``--host-queries``
  query rows against all references, wall clock; ``host_extrapolated_ms`` scales that linearly to all nq queries and is marked as
  an extrapolation -- the restatement at the full size is not run;
* ``same_integers``: whether the device's neighbours of those first queries equal the restatement's;
* ``gru_forward``: wall clock of ONE forward pass (``predict_proba``) of a cfg3 GRU (bench.py: cfg3gru -- embedding 512, hidden
  512, 4 layers, batch 50) with untrained weights over the same query rows (2 warm-up, 5 samples).

``--ab NAME`` (a run of its own, whose parent process never opens the GPU; with ``--out`` it is merged into that file under
``edit_knn_rows_<shape>_vs_parent``): ``ops.edit_knn_rows`` at 4000 x 4000 and at 16384 x 4000 under the product library and under
lib/libslnlp_probeNAME.so (the parent commit's tree built with ``make VARIANT=NAME``), in fresh child processes, interleaved,
``--ab-rounds`` times on this box (tools/knn_ab.py): each child's batched median, and per build the spread between its repeated
medians.  The margin is the parent's own spread.

No pass / fail: the numbers are recorded."""
import argparse
import json
import os
import sys
import time

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from time_field_knn import emit

S, K, SRC_VOCAB, LABELS = 48, 5, 3000, 200
SHAPES = (("test_vs_train_800x3200", 800, 3200), ("leave_one_out_4000x4000", 4000, 4000), ("large_16384x4000", 16384, 4000))
WARMUP, SAMPLES, BATCH = 5, 30, 10
CFG = dict(E=512, Hd=512, layers=4, B=50)


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


def sampled(fn):
    lone = stats([timed_us(fn) for _ in range(WARMUP + SAMPLES)][WARMUP:], "us")
    batched = stats([timed_us(fn, BATCH) for _ in range(3 + 10)][3:], "us")
    return lone, batched


def time_shape(name, nq, nr, data, host_queries, gru):
    import edit_knn_ref as R
    import slnlp
    from slnlp import ops
    print(f"[time_edit_knn] {name} ...", file=sys.stderr, flush=True)
    train, test = data[np.arange(nr)], data[np.arange(nr, nr + nq)]
    V = len(data.vocab_y)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Xq, Lq, Xr, Lr, yr = dev(test.ids), dev(test.lengths), dev(train.ids), dev(train.lengths), dev(train.y)
    prior = dev(R.prior_of(train.y, V))
    dist = torch.empty(nq, nr, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(nq * nr, dtype=torch.uint8, device="cuda")
    buf = ops.edit_knn_buffers(nq, K, "cuda")
    logp = torch.empty(nq, V, dtype=torch.float32, device="cuda")
    res = {"name": name, "nq": nq, "nr": nr, "S": S, "k": K, "V": V, "pairs": nq * nr, "scratch_bytes": nq * nr}
    for key, fn in (("distances", lambda: ops.edit_distances(Xq, Lq, Xr, Lr, out=dist)),
                    ("knn_rows", lambda: ops.edit_knn_rows(Xq, Lq, Xr, Lr, K, buf=buf, scratch=scratch)),
                    ("knn_logp", lambda: ops.edit_knn_logp(buf, Lq, Lr, yr, prior, out=logp))):
        res[key], res[key + "_batched"] = sampled(fn)
    res["pairs_per_us"] = nq * nr / res["distances_batched"]["median_us"]
    knn = slnlp.EditKNN(k=K).fit(train)
    res["predict_proba"] = stats([wall_ms(lambda: knn.predict_proba(test))[0] for _ in range(3 + 10)][3:], "ms")
    m = min(host_queries, nq)

    def host():
        d = R.distances(test.ids[:m], test.lengths[:m], train.ids, train.lengths)
        got = R.knn_rows(d, test.lengths[:m], train.lengths, S, S, K)
        return got, R.knn_logp(got, test.lengths[:m], train.lengths, train.y, R.prior_of(train.y, V))[0]
    t0 = time.perf_counter()
    want, _ = host()
    host_ms = (time.perf_counter() - t0) * 1e3
    got = ops.edit_knn_download(buf)
    res["host"] = {"queries_timed": m, "ms": host_ms, "host_extrapolated_ms": host_ms * nq / m,
                   "note": f"the restatement was run on the first {m} of {nq} queries; host_extrapolated_ms is that time x {nq}/{m}, not a run"}
    res["same_integers"] = bool(np.array_equal(got["nbr"][:m], want["nbr"]) and np.array_equal(got["rows"][:m], want["rows"]))
    res["extrapolated_host_over_predict_proba"] = res["host"]["host_extrapolated_ms"] / res["predict_proba"]["median_ms"]
    try:
        res["gru_forward"] = stats([wall_ms(lambda: gru.predict_proba(test))[0] for _ in range(2 + 5)][2:], "ms")
        res["gru_forward_over_predict_proba"] = res["gru_forward"]["median_ms"] / res["predict_proba"]["median_ms"]
    except Exception as e:                                   # recorded as what it is: no number
        res["gru_forward"] = {"not_measured": f"{type(e).__name__}: {e}"}
    return res


def ab_child(nq, nr):
    """One child of the A / B: edit_knn_rows at nq x nr, batched medians of its own repeats"""
    from slnlp import ops
    from slnlp.data import synthetic_dataset
    data = synthetic_dataset(nq + nr, seq_len=S, src_vocab=SRC_VOCAB, n_labels=LABELS, seed=1, min_len=8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Xr, Lr, Xq, Lq = dev(data.ids[:nr]), dev(data.lengths[:nr]), dev(data.ids[nr:]), dev(data.lengths[nr:])
    buf = ops.edit_knn_buffers(nq, K, "cuda")
    scratch = torch.empty(nq * nr, dtype=torch.uint8, device="cuda")
    fn = lambda: ops.edit_knn_rows(Xq, Lq, Xr, Lr, K, buf=buf, scratch=scratch)
    batched = stats([timed_us(fn, 4) for _ in range(2 + 9)][2:], "us")
    got = ops.edit_knn_download(buf)
    print(json.dumps({"knn_rows_batched": batched, "checksum": int(got["nbr"].astype(np.int64).sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-queries", type=int, default=8)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    ap.add_argument("--ab", default=None, help="NAME of lib/libslnlp_probeNAME.so, the parent commit's library")
    ap.add_argument("--ab-rounds", type=int, default=4)
    ap.add_argument("--ab-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.ab:                                              # children only: this process stays off the GPU
        from knn_ab import ab
        res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        for name, nq, nr in SHAPES[1:]:
            what = (f"ops.edit_knn_rows (distances, selection, head) at {nq} x {nr}, S = {S}, k = {K}; 4 calls between one pair of events, median of 9 "
                    "repeats per child process; children interleaved on one box")
            res[f"edit_knn_rows_{nq}x{nr}_vs_parent"] = ab(HERE, ["--ab-child", f"{nq}x{nr}"], args.ab, args.ab_rounds, what, "time_edit_knn")
        return emit(res, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_edit_knn.py: no GPU -- nothing is measured without one")
    if args.ab_child:
        return ab_child(*(int(v) for v in args.ab_child.split("x")))
    from slnlp.data import synthetic_dataset
    from slnlp.net import NeuralNetClassifier
    which = [SHAPES[int(i)] for i in args.shapes.split(",")] if args.shapes else list(SHAPES)
    rows = max(nq + nr for _, nq, nr in which)
    data = synthetic_dataset(rows, seq_len=S, src_vocab=SRC_VOCAB, n_labels=LABELS, seed=1, min_len=8)
    gru = NeuralNetClassifier(module="model.EncoderDecoderGRUAttn", module__embedding_size=CFG["E"], module__hidden_size=CFG["Hd"],
                              module__num_layers=CFG["layers"], module__dropout=0.1, module__src_vocab=data.vocab_X, module__tgt_vocab=data.vocab_y,
                              module__batch_first=True, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1, optimizer="torch.optim.SGD",
                              optimizer__momentum=0.9, lr=0.05, max_epochs=1, batch_size=CFG["B"], device="cuda",
                              gradient_clipping={"gradient_clip_value": 0.5})
    torch.manual_seed(1)
    gru.initialize()
    gru.classes_ = np.arange(len(data.vocab_y))
    res = {"command": "python tools/time_edit_knn.py --out profiles/edit_knn_timing.json", "device": torch.cuda.get_device_name(0),
           "shapes": [time_shape(name, nq, nr, data, args.host_queries, gru) for name, nq, nr in which],
           "gru": {"model": "cfg3gru, untrained weights", **CFG, "S": S, "labels": LABELS},
           "note": ("distances / knn_rows / knn_logp: HIP events around one ops call (1 / 3 / 2 launches), the second event waited for, "
                    f"{SAMPLES} samples after {WARMUP} warm-up; *_batched: {BATCH} calls between one pair of events, per call; predict_proba and "
                    "gru_forward: wall clock between two device synchronisations; host: the numpy restatement on a stated subset of the "
                    "queries, host_extrapolated_ms scaled linearly and NOT measured at the full size")}
    emit(res, args.out)


if __name__ == "__main__":
    main()
