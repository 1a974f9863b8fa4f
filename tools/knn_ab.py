"""The A / B of one neighbour-search call against the parent commit's library, shared by the ``--ab NAME`` mode of
tools/time_edit_knn.py, tools/time_edit_long.py and tools/time_field_weights.py (not run by itself).

The parent process never opens the GPU.  It starts the tool again as a child (``child_args``) under the product library and under
lib/libslnlp_probeNAME.so (the parent commit's tree built with ``make VARIANT=NAME``; the child loads it through
``SLNLP_PROBE_LIB=NAME``), in fresh processes, interleaved, ``rounds`` times on one box.  A child prints one JSON line
{"knn_rows_batched": {"median_us": ...}, "checksum": ...}: the batched median of its own repeats and a sum over the neighbours it
found.  Per build: the medians, their median and THE SPREAD between the repeated medians (max - min); the margin of the comparison
is the parent's own spread -- what this box cannot tell apart."""
import json
import os
import subprocess
import sys

import numpy as np


def ab(here, child_args, name, rounds, what, tag, timeout=300):
    res = {"product": [], name: []}
    for r in range(rounds):
        for variant in (name, "product"):
            env = dict(os.environ)
            env.pop("SLNLP_PROBE_LIB", None)
            if variant != "product":
                env["SLNLP_PROBE_LIB"] = variant
            out = subprocess.run([sys.executable, here, *child_args], env=env, capture_output=True, text=True, timeout=timeout)
            if out.returncode != 0:
                raise SystemExit(f"{tag} --ab: the {variant} child failed ({out.returncode}): {out.stderr[-600:]}")
            res[variant].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(f"[{tag}] ab round {r} {variant}: {res[variant][-1]['knn_rows_batched']['median_us']:.1f} us", file=sys.stderr, flush=True)
    out = {"what": what, "command": " ".join(["python", os.path.relpath(here, os.path.dirname(os.path.dirname(here))), "--ab", name]), "rounds": rounds}
    for variant, runs in res.items():
        med = [c["knn_rows_batched"]["median_us"] for c in runs]
        out[variant] = {"medians_us": med, "median_of_medians_us": float(np.median(med)), "spread_us": float(max(med) - min(med)),
                        "checksums": [c["checksum"] for c in runs]}
    out["difference_us"] = out["product"]["median_of_medians_us"] - out[name]["median_of_medians_us"]
    out["margin_us"] = out[name]["spread_us"]
    out["within_margin"] = bool(abs(out["difference_us"]) <= out["margin_us"])
    out["not_slower_beyond_margin"] = bool(out["difference_us"] <= out["margin_us"])
    out["same_neighbours"] = len({c for v in ("product", name) for c in out[v]["checksums"]}) == 1
    return out
