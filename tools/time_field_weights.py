"""Cost of the per-field weighted edit distance and of the search that fits the weights (``slnlp_field_distances_w`` /
``slnlp_field_knn_rows_w`` / ``slnlp_loo_objective``: ``slnlp.PhonoKNN(field_weights=)``, ``slnlp.fit_field_weights``), and the A / B
of the untouched unweighted ``field_knn_rows`` against the parent commit's library.

    python tools/time_field_weights.py [--out profiles/field_weights_timing.json]
    python tools/time_field_weights.py --ab parent [--out profiles/field_weights_timing.json]

Rows of S = 48 positions from ``synthetic_dataset`` (3000 source tokens, 200 labels, lengths 8..48), F = 6 fields (a made-up table:
token v's codes are the six base-4 digits of v), k = 5.  In one process on one stream:

* ``distances``: at 800 x 3200 and 4000 x 4000, ``field_distances`` (unweighted, gap 6), ``field_distances(field_weights=ones)``
  (gap 6) and ``field_distances(field_weights=(4, 0, 2, 0, 1, 3))`` (gap 10), INTERLEAVED -- one call of each in turn between its
  own pair of HIP events, the second event waited for -- medians of the samples, and the ratios to the unweighted median;
* ``search``: ``fit_field_weights`` at N = 4000 with the default levels and sweeps, wall clock between two device
  synchronisations, its evaluations and the time per evaluation; beside it one ``PhonoKNN.leave_one_out()`` pass of the same rows
  (``_forward_logp`` to a device tensor) in the same run.  The synthetic tokens carry no field structure: the search's RESULT here
  means nothing, only its cost does.

``--ab NAME`` (a run of its own, whose parent process never opens the GPU; with ``--out`` it is merged into that file under
``field_knn_rows_vs_parent``): the unweighted ``field_knn_rows`` at 4000 x 4000 under the product library and under
lib/libslnlp_probeNAME.so (the parent commit's tree built with ``make VARIANT=NAME``), in fresh child processes, interleaved,
``--ab-rounds`` times on this box: each child's batched median, and per build the spread between its repeated medians.  The margin
is the parent's own spread.

No claim is made about real ASL-Phono data: whether fitted weights beat unit weights there is what ``phono_vs_weighted`` (the CLI
key ``phono_baseline.fit_weights``) tells a user on their own data.  No pass / fail: the numbers are recorded."""
import argparse
import json
import os
import sys
import time

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from time_field_knn import F, K, LABELS, S, SRC_VOCAB, emit, field_table, stats, timed_us, wall_ms

WEIGHTS = (4, 0, 2, 0, 1, 3)
SHAPES = (("test_vs_train_800x3200", 800, 3200), ("leave_one_out_4000x4000", 4000, 4000))


def time_distances(name, nq, nr, data, samples=12, warmup=3):
    from slnlp import ops
    print(f"[time_field_weights] distances {name} ...", file=sys.stderr, flush=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Xr, Lr, Xq, Lq = dev(data.ids[:nr]), dev(data.lengths[:nr]), dev(data.ids[nr:nr + nq]), dev(data.lengths[nr:nr + nq])
    codes = dev(field_table())
    out = torch.empty(nq, nr, dtype=torch.uint16, device="cuda")
    calls = {"unweighted": lambda: ops.field_distances(Xq, Lq, Xr, Lr, codes, F, out=out),
             "weighted_ones": lambda: ops.field_distances(Xq, Lq, Xr, Lr, codes, F, out=out, field_weights=(1,) * F),
             "weighted": lambda: ops.field_distances(Xq, Lq, Xr, Lr, codes, sum(WEIGHTS), out=out, field_weights=WEIGHTS)}
    us = {key: [] for key in calls}
    for _ in range(warmup + samples):                        # interleaved: one call of each in turn
        for key, fn in calls.items():
            us[key].append(timed_us(fn))
    res = {"name": name, "nq": nq, "nr": nr, "S": S, "F": F, "weights": list(WEIGHTS), "samples": samples}
    for key in calls:
        res[key] = stats(us[key][warmup:], "us")
    for key in ("weighted_ones", "weighted"):
        res[f"{key}_over_unweighted"] = res[key]["median_us"] / res["unweighted"]["median_us"]
    a = ops.field_distances(Xq, Lq, Xr, Lr, codes, F).cpu().numpy()
    b = ops.field_distances(Xq, Lq, Xr, Lr, codes, F, field_weights=(1,) * F).cpu().numpy()
    res["ones_equal_unweighted_bytes"] = bool(a.tobytes() == b.tobytes())
    return res


def time_search(data, N=4000):
    import slnlp
    print("[time_field_weights] the search ...", file=sys.stderr, flush=True)
    train = data[np.arange(N)]
    table = field_table()
    loo = slnlp.PhonoKNN(table, k=K).fit(train).leave_one_out()
    one = lambda: loo._forward_logp(train, lambda z, y: z)
    passes = stats([wall_ms(one)[0] for _ in range(2 + 5)][2:], "ms")
    ms, rep = wall_ms(lambda: slnlp.fit_field_weights(train, table, k=K))
    ms2, rep2 = wall_ms(lambda: slnlp.fit_field_weights(train, table, k=K))
    return {"N": N, "F": F, "k": K, "levels": [0, 1, 2, 4], "sweeps": 2, "scoring": "neg_log_loss", "wall_ms_first": ms, "wall_ms": ms2,
            "evaluations": rep2["evaluations"], "ms_per_evaluation": ms2 / rep2["evaluations"], "sweeps_run": rep2["sweeps_run"], "converged": rep2["converged"],
            "weights": list(rep2["weights"]), "same_result_twice": bool(rep["trace"] == rep2["trace"]), "leave_one_out_pass": passes,
            "note": "wall clock between two device synchronisations; leave_one_out_pass: one PhonoKNN.leave_one_out()._forward_logp of the same rows "
                    "(unit weights) in the same process; the synthetic tokens carry no field structure, so the fitted weights mean nothing here"}


def ab_child():
    """One child of the A / B: the unweighted field_knn_rows at 4000 x 4000, batched medians of its own repeats"""
    from slnlp import ops
    from slnlp.data import synthetic_dataset
    nq = nr = 4000
    data = synthetic_dataset(nq + nr, seq_len=S, src_vocab=SRC_VOCAB, n_labels=LABELS, seed=1, min_len=8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Xr, Lr, Xq, Lq = dev(data.ids[:nr]), dev(data.lengths[:nr]), dev(data.ids[nr:]), dev(data.lengths[nr:])
    codes = dev(field_table())
    buf = ops.edit_knn_buffers(nq, K, "cuda")
    scratch = torch.empty(2 * nq * nr, dtype=torch.uint8, device="cuda")
    fn = lambda: ops.field_knn_rows(Xq, Lq, Xr, Lr, codes, K, gap=F, buf=buf, scratch=scratch)
    batched = stats([timed_us(fn, 4) for _ in range(2 + 9)][2:], "us")
    got = ops.edit_knn_download(buf)
    print(json.dumps({"knn_rows_batched": batched, "checksum": int(got["nbr"].astype(np.int64).sum())}))


def ab(name, rounds):
    """tools/knn_ab.py: the children interleaved, each build's medians and spread"""
    from knn_ab import ab as ab_children
    what = ("ops.field_knn_rows WITHOUT weights (distances, selection, head) at 4000 x 4000, S = 48, F = 6, k = 5; 4 calls between one pair of "
            "events, median of 9 repeats per child process; children interleaved on one box")
    return ab_children(HERE, ["--ab-child"], name, rounds, what, "time_field_weights")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", default=None, help="NAME of lib/libslnlp_probeNAME.so, the parent commit's library")
    ap.add_argument("--ab-rounds", type=int, default=4)
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.ab:                                              # children only: this process stays off the GPU
        res = {}
        if args.out and os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["field_knn_rows_vs_parent"] = ab(args.ab, args.ab_rounds)
        return emit(res, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_field_weights.py: no GPU -- nothing is measured without one")
    if args.ab_child:
        return ab_child()
    from slnlp.data import synthetic_dataset
    data = synthetic_dataset(8000, seq_len=S, src_vocab=SRC_VOCAB, n_labels=LABELS, seed=1, min_len=8)
    res = {"command": "python tools/time_field_weights.py --out profiles/field_weights_timing.json; then the same with --ab parent",
           "device": torch.cuda.get_device_name(0),
           "distances": [time_distances(name, nq, nr, data) for name, nq, nr in SHAPES],
           "search": time_search(data),
           "not_claimed": "nothing about real ASL-Phono data: whether fitted weights beat unit weights there is what phono_vs_weighted "
                          "(phono_baseline.fit_weights) tells a user on their own data"}
    emit(res, args.out)


if __name__ == "__main__":
    main()
