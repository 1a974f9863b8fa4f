"""Cost of the phonology-weighted neighbour search on the device (``slnlp_field_distances`` / ``slnlp_field_knn_rows`` /
``slnlp_field_knn_logp``: ``slnlp.PhonoKNN``), beside the unit-cost search re-measured in the same run, and the A / B of the
unit-cost ``edit_knn_rows`` against the parent commit's library (the selection body became generic).

    python tools/time_field_knn.py [--out profiles/field_knn_timing.json] [--host-queries 8]
    python tools/time_field_knn.py --ab parent [--out profiles/field_knn_timing.json]

Rows of S = 48 positions from ``synthetic_dataset`` (3000 source tokens, 200 labels, lengths 8..48), F = 6 fields (a made-up table:
token v's codes are the six base-4 digits of v), gap = F, k = 5, at 800 x 3200, 4000 x 4000 and 16384 x 4000 (queries x
references).  In one process on one stream, per shape:

* ``field`` and ``unit``: ``distances``, ``knn_rows``, ``knn_logp`` -- one ``ops`` call each (1 / 3 / 2 launches) between two HIP
  events, the second one waited for, into buffers allocated once; warm-up calls, then samples; ``*_batched``: several calls between
  one pair of events, per call.  Medians, minima and maxima of the repeats are kept;
* ``cell_updates_per_s``: the DP cells of all usable pairs (sum of len(query) x len(reference)) over ``field.distances_batched``'s
  median; ``valu_share``: that rate x ``VALU_PER_CELL`` over the device's integer VALU rate (256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz).
  ``VALU_PER_CELL`` is read from the gfx950 ISA of ``field_dist_kernel_g2`` (F = 5..8: two groups of four fields), whose loop over
  a column word -- two cells -- is one block of 76 instructions: 55 vector ALU, 8 LDS, 8 scalar ALU, 4 waits and a branch, i.e.
  27.5 vector ALU instructions a cell of 38 issued;
* ``predict_proba``: wall clock between two device synchronisations of ``PhonoKNN.predict_proba`` / ``EditKNN.predict_proba``;
* ``host``: the numpy restatement (tests/field_knn_ref.py: distances, selection, vote) on the FIRST ``--host-queries`` query rows
  against all references, wall clock -- stated as what it is, not scaled to the full size; ``same_integers``: whether the device's
  neighbours of those queries equal the restatement's.

``--ab NAME`` (a run of its own, whose parent process never opens the GPU; with ``--out`` it is merged into that file under
``edit_knn_rows_vs_parent``): the unit-cost ``edit_knn_rows`` at 4000 x 4000 under the product library and under lib/libslnlp_probeNAME.so (the
parent commit's tree built with ``make VARIANT=NAME``), in fresh child processes, interleaved, ``--ab-rounds`` times on this box:
each child's batched median, and per build the spread between its repeated medians.  The margin is the parent's own spread.

No pass / fail: the numbers are recorded."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

S, K, F, SRC_VOCAB, LABELS = 48, 5, 6, 3000, 200
SHAPES = (("test_vs_train_800x3200", 800, 3200), ("leave_one_out_4000x4000", 4000, 4000), ("large_16384x4000", 16384, 4000))
VALU_PER_CELL, ISSUED_PER_CELL = 27.5, 38
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


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


def sampled(fn, warmup, samples, batch, repeats):
    lone = stats([timed_us(fn) for _ in range(warmup + samples)][warmup:], "us")
    batched = stats([timed_us(fn, batch) for _ in range(2 + repeats)][2:], "us")
    return lone, batched


def field_table():
    v = np.arange(SRC_VOCAB + 2)
    return np.stack([(v // 4 ** f) % 4 for f in range(F)], axis=1).astype(np.int32)


def time_shape(name, nq, nr, data, host_queries):
    import field_knn_ref as R
    import slnlp
    from slnlp import ops
    print(f"[time_field_knn] {name} ...", file=sys.stderr, flush=True)
    train, test = data[np.arange(nr)], data[np.arange(nr, nr + nq)]
    V = len(data.vocab_y)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Xq, Lq, Xr, Lr, yr = dev(test.ids), dev(test.lengths), dev(train.ids), dev(train.lengths), dev(train.y)
    table = field_table()
    codes = dev(table)
    prior = dev(R.prior_of(train.y, V))
    buf = ops.edit_knn_buffers(nq, K, "cuda")
    logp = torch.empty(nq, V, dtype=torch.float32, device="cuda")
    cells = int(test.lengths.sum()) * int(train.lengths.sum())
    res = {"name": name, "nq": nq, "nr": nr, "S": S, "k": K, "F": F, "gap": F, "V": V, "pairs": nq * nr, "cells": cells}
    dist16 = torch.empty(nq, nr, dtype=torch.uint16, device="cuda")
    scratch16 = torch.empty(2 * nq * nr, dtype=torch.uint8, device="cuda")
    heavy = dict(warmup=2, samples=8, batch=4, repeats=5)
    light = dict(warmup=5, samples=30, batch=10, repeats=10)
    res["field"] = {"scratch_bytes": 2 * nq * nr}
    for key, fn, how in (("distances", lambda: ops.field_distances(Xq, Lq, Xr, Lr, codes, F, out=dist16), heavy),
                         ("knn_rows", lambda: ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, K, gap=F, buf=buf, scratch=scratch16), heavy),
                         ("knn_logp", lambda: ops.field_knn_logp(buf, Lq, Lr, yr, prior, F, out=logp), light)):
        res["field"][key], res["field"][key + "_batched"] = sampled(fn, **how)
    field_nbr = {n: v.copy() for n, v in ops.edit_knn_download(buf).items()}
    sec = res["field"]["distances_batched"]["median_us"] * 1e-6
    res["cell_updates_per_s"] = cells / sec
    res["valu_share"] = {"valu_per_cell": VALU_PER_CELL, "issued_per_cell": ISSUED_PER_CELL, "device_valu_lane_ops_per_s": VALU_LANE_OPS_PER_S,
                         "share": cells / sec * VALU_PER_CELL / VALU_LANE_OPS_PER_S}
    del dist16, scratch16
    dist8 = torch.empty(nq, nr, dtype=torch.uint8, device="cuda")
    scratch8 = torch.empty(nq * nr, dtype=torch.uint8, device="cuda")
    res["unit"] = {"scratch_bytes": nq * nr}
    for key, fn in (("distances", lambda: ops.edit_distances(Xq, Lq, Xr, Lr, out=dist8)),
                    ("knn_rows", lambda: ops.edit_knn_rows(Xq, Lq, Xr, Lr, K, buf=buf, scratch=scratch8)),
                    ("knn_logp", lambda: ops.edit_knn_logp(buf, Lq, Lr, yr, prior, out=logp))):
        res["unit"][key], res["unit"][key + "_batched"] = sampled(fn, **light)
    del dist8, scratch8
    phono = slnlp.PhonoKNN(table, k=K).fit(train)
    unit = slnlp.EditKNN(k=K).fit(train)
    res["field"]["predict_proba"] = stats([wall_ms(lambda: phono.predict_proba(test))[0] for _ in range(2 + 6)][2:], "ms")
    res["unit"]["predict_proba"] = stats([wall_ms(lambda: unit.predict_proba(test))[0] for _ in range(2 + 6)][2:], "ms")
    m = min(host_queries, nq)
    t0 = time.perf_counter()
    d = R.distances(test.ids[:m], test.lengths[:m], train.ids, train.lengths, table, F)
    want = R.knn_rows(d, test.lengths[:m], train.lengths, S, S, K, F)
    R.knn_logp(want, test.lengths[:m], train.lengths, train.y, R.prior_of(train.y, V), F)
    res["host"] = {"queries_timed": m, "ms": (time.perf_counter() - t0) * 1e3,
                   "note": f"the numpy restatement on the first {m} of {nq} queries against all {nr} references; not run and not scaled to the full size"}
    res["same_integers"] = bool(np.array_equal(field_nbr["nbr"][:m], want["nbr"]) and np.array_equal(field_nbr["rows"][:m], want["rows"]))
    return res


def ab_child():
    """One child of the A / B: the unit-cost edit_knn_rows at 4000 x 4000, batched medians of its own repeats"""
    from slnlp import ops
    from slnlp.data import synthetic_dataset
    nq = nr = 4000
    data = synthetic_dataset(nq + nr, seq_len=S, src_vocab=SRC_VOCAB, n_labels=LABELS, seed=1, min_len=8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Xr, Lr, Xq, Lq = dev(data.ids[:nr]), dev(data.lengths[:nr]), dev(data.ids[nr:]), dev(data.lengths[nr:])
    buf = ops.edit_knn_buffers(nq, K, "cuda")
    scratch = torch.empty(nq * nr, dtype=torch.uint8, device="cuda")
    fn = lambda: ops.edit_knn_rows(Xq, Lq, Xr, Lr, K, buf=buf, scratch=scratch)
    _, batched = sampled(fn, warmup=5, samples=5, batch=20, repeats=15)
    got = ops.edit_knn_download(buf)
    print(json.dumps({"knn_rows_batched": batched, "checksum": int(got["nbr"].astype(np.int64).sum())}))


def ab(name, rounds):
    res = {"product": [], name: []}
    for r in range(rounds):
        for variant in (name, "product"):
            env = dict(os.environ)
            env.pop("SLNLP_PROBE_LIB", None)
            if variant != "product":
                env["SLNLP_PROBE_LIB"] = variant
            out = subprocess.run([sys.executable, HERE, "--ab-child"], env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                raise SystemExit(f"time_field_knn --ab: the {variant} child failed: {out.stderr[-600:]}")
            res[variant].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(f"[time_field_knn] ab round {r} {variant}: {res[variant][-1]['knn_rows_batched']['median_us']:.1f} us", file=sys.stderr, flush=True)
    out = {"what": "ops.edit_knn_rows (unit-cost: distances, selection, head) at 4000 x 4000, S = 48, k = 5; 20 calls between one pair of events, "
                   "median of 15 repeats per child process; children interleaved on one box", "rounds": rounds}
    for variant, runs in res.items():
        med = [c["knn_rows_batched"]["median_us"] for c in runs]
        out[variant] = {"medians_us": med, "median_of_medians_us": float(np.median(med)), "spread_us": float(max(med) - min(med)),
                        "checksums": [c["checksum"] for c in runs]}
    out["difference_us"] = out["product"]["median_of_medians_us"] - out[name]["median_of_medians_us"]
    out["margin_us"] = out[name]["spread_us"]
    out["within_margin"] = bool(out["difference_us"] <= out["margin_us"])
    out["same_neighbours"] = len({c for v in ("product", name) for c in out[v]["checksums"]}) == 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-queries", type=int, default=8)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    ap.add_argument("--ab", default=None, help="NAME of lib/libslnlp_probeNAME.so, the parent commit's library")
    ap.add_argument("--ab-rounds", type=int, default=4)
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.ab:                                              # children only: this process stays off the GPU
        res = {}
        if args.out and os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["edit_knn_rows_vs_parent"] = ab(args.ab, args.ab_rounds)
        return emit(res, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_field_knn.py: no GPU -- nothing is measured without one")
    if args.ab_child:
        return ab_child()
    from slnlp.data import synthetic_dataset
    which = [SHAPES[int(i)] for i in args.shapes.split(",")] if args.shapes else list(SHAPES)
    rows = max(nq + nr for _, nq, nr in which)
    data = synthetic_dataset(rows, seq_len=S, src_vocab=SRC_VOCAB, n_labels=LABELS, seed=1, min_len=8)
    res = {"command": "python tools/time_field_knn.py --out profiles/field_knn_timing.json; then the same with --ab parent", "device": torch.cuda.get_device_name(0),
           "host_name": os.uname().nodename,
           "shapes": [time_shape(name, nq, nr, data, args.host_queries) for name, nq, nr in which],
           "note": ("distances / knn_rows / knn_logp: HIP events around one ops call (1 / 3 / 2 launches), the second event waited for; *_batched: "
                    "several calls between one pair of events, per call; medians of the repeats; field.* is the phonology-weighted search (F = 6, "
                    "gap = 6), unit.* the unit-cost search re-measured in the same process; predict_proba: wall clock between two device "
                    "synchronisations; host: the numpy restatement on a stated subset of the queries, NOT scaled to the full size; valu_share: "
                    "cell_updates_per_s x valu_per_cell (read from the ISA at F = 6) over 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz")}
    emit(res, args.out)


def emit(res, out):
    line = json.dumps(res, indent=1)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
