#!/usr/bin/env python3
"""Host cost of the packed judging buffers: ``*_buffers`` plus ``*_download`` for each of the eleven, timed with ``timeit`` on the
CPU device (no copy, no launch: what is left is the Python that lays the pieces out and cuts them), at the shapes the tools/time_*.py
use -- N = 4000 rows, V = 202 classes, k = 5, 20 pairs, 15 bins, 1000 replicates, 40000 variants in 8 bins.

    python tools/time_packed_host.py [--against OLD_TREE] [--out profiles/packed_buffers_host.json]

``--against``: the root of another checkout (built), whose ``slnlp`` is loaded beside this tree's in the SAME process; every repeat
times CALLS calls of the one and then of the other, so that both meet the same state of the machine, and the difference is formed per
repeat.  One JSON object {name: {"this": {"us": median microseconds per call pair, "min", "max"}, "other": ..., "delta_us": ...}}.
"""
import argparse
import json
import os
import statistics
import sys
import timeit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd")):
    sys.path.insert(0, p)

N, V, K, PAIRS, BINS, B, VARIANTS, VAR_BINS = 4000, 202, 5, 20, 15, 1000, 40000, 8
CALLS, REPEATS = 100, 25


def pairs(ops, np):
    variants = np.stack([np.arange(VARIANTS) % N, np.arange(VARIANTS) // N, np.arange(VARIANTS) % VAR_BINS], axis=1).astype(np.int32)
    start = np.minimum(np.arange(N + 1) * 10, VARIANTS).astype(np.int32)
    return {"score": lambda: ops.score_download(ops.score_buffers(N, V, "cpu")),
            "reliability": lambda: ops.reliability_download(ops.reliability_buffers(N, BINS, "cpu")),
            "ranking": lambda: ops.ranking_download(ops.ranking_buffers(N, V, "cpu"), per_row=True),
            "topk": lambda: ops.topk_download(ops.topk_buffers(N, K, "cpu")),
            "conformal": lambda: ops.conformal_download(ops.conformal_buffers(N, V, "cpu"), rows=True, sets=True),
            "selective": lambda: ops.selective_download(ops.selective_buffers(N, "cpu")),
            "error_analysis": lambda: ops.error_analysis_download(ops.error_analysis_buffers(N, V, K, PAIRS, "cpu"), matrix=True, topk=True),
            "label_audit": lambda: ops.label_audit_download(ops.label_audit_buffers(N, V, PAIRS, "cpu"), per_row=True),
            "attribution": lambda: ops.attribution_download(ops.attribution_buffers(N, V, variants, start, VAR_BINS, "cpu"), per_variant=True),
            "bootstrap": lambda: ops.bootstrap_download(ops.bootstrap_buffers(B, V, 3, True, "cpu")),
            "score_interval": lambda: ops.score_interval_download(ops.score_interval_buffers(N, V, B, "cpu", bins=BINS))}


def package(tree, name):
    """the ``slnlp`` package of the checkout ``tree`` under the module name ``name``"""
    import importlib.util
    where = os.path.join(tree, "sign-language-nlp_amd", "slnlp")
    spec = importlib.util.spec_from_file_location(name, os.path.join(where, "__init__.py"), submodule_search_locations=[where])
    sys.modules[name] = module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return importlib.import_module(name + ".ops"), importlib.import_module(name + ".metrics")


def summary(us):
    return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(1)
    trees = {"this": package(ROOT, "slnlp")}
    if args.against:
        trees["other"] = package(os.path.abspath(args.against), "slnlp_other")
    calls = {}
    for label, (ops, metrics) in trees.items():
        metrics.reliability_from_table = metrics.ranking_from_table = lambda table: {}     # the cut, not the scores of an unwritten table
        calls[label] = pairs(ops, np)
    got = {"shapes": {"N": N, "V": V, "k": K, "pairs": PAIRS, "bins": BINS, "replicates": B, "variants": VARIANTS, "variant_bins": VAR_BINS,
                      "calls": CALLS, "repeats": REPEATS, "unit": "microseconds per *_buffers + *_download pair, CPU device"}}
    for name in calls["this"]:
        us = {label: [] for label in calls}
        for _ in range(REPEATS + 1):                         # (the first repeat warms both up)
            for label in calls:
                us[label].append(timeit.timeit(calls[label][name], number=CALLS) / CALLS * 1e6)
        got[name] = {label: summary(v[1:]) for label, v in us.items()}
        if args.against:
            got[name]["delta_us"] = summary([a - b for a, b in zip(us["this"][1:], us["other"][1:])])
    print(json.dumps(got))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(got, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
