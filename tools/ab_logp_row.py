#!/usr/bin/env python3
"""The log-prob judging kernels that share a header of csrc/ (logp_row.hpp, block_reduce.hpp, rank_chunk.hpp), timed against another
build of the library on ONE box: each feature's existing timer (tools/time_reliability.py, time_error_analysis.py, time_conformal.py,
time_ranking.py, time_selective.py, time_prior_shift.py, time_calibration.py: their own shapes, samples and HIP events) and, for
the ensemble, HIP events around ``ops.ensemble_rows`` at 4000 x 202 with K = 5 -- every one in a fresh child process, the two
libraries alternating, `--rounds` times.  Three more workloads stand for the kernels that share the wave-per-row loop and the
queued fits' state (csrc/common.hpp: wave_rows, csrc/fit_state.hpp): `bias_calibration` (tools/time_bias_calibration.py: the whole
queued fit), `label_audit` (tools/time_label_audit.py: the audit's eight launches, its joint stages, scatter_logp and scale_logp)
and `epoch_scoring` (tools/time_epoch_scoring.py: the wall clock of an epoch end on score_rows, in microseconds like the rest).

    python tools/ab_logp_row.py --variant parent [--rounds 5] [--workloads ranking selective ...] [--out profiles/logp_row_ab.json]
        parent = lib/libslnlp_probeparent.so (make VARIANT=parent in a checkout of the old tree)
        --workloads: a subset of the eleven (default: all)

Per figure (median microseconds of one child): every round's value for both builds, the parent's min..max over its rounds, the new
build's median over its rounds and whether that lies inside the parent's spread -- the only yardstick there is for kernels nobody
has timed across a code-motion change."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
WORKLOADS = ("reliability", "topk", "conformal", "ensemble", "ranking", "selective", "prior_shift", "calibration", "bias_calibration",
             "label_audit", "epoch_scoring")


def child(workload):
    """-> {figure: median us} of the kernel under test, from the feature's own timer"""
    import torch
    if workload == "reliability":
        import time_reliability as t
        out = {}
        for N, V in t.SHAPES:
            res = t.time_shape(N, V)
            for k in ("reliability_rows", "reliability_rows_state_1", "reliability_rows_beta"):
                out[f"{k}_{N}x{V}"] = res["back_to_back"][k]["median_us"]
        return out
    if workload == "topk":
        import time_error_analysis as t
        return {f"topk_rows_{N}x{V}": t.time_shape(N, V)["topk_rows"]["median_us"] for N, V in t.SHAPES}
    if workload == "conformal":
        import time_conformal as t
        res = t.time_kernel_and_routes()
        return {f"conformal_{k}{suffix}": res[part][k]["median_us"] for k in ("rows_scores", "rows_sets")
                for part, suffix in (("kernel", ""), ("kernel_batched", "_batched"))}
    if workload == "ranking":
        import time_ranking as t
        res = t.time_kernel_and_routes()
        return {f"ranking_rows_{k}{suffix}": res[part][k]["median_us"] for k in ("table_only", "with_rows")
                for part, suffix in (("kernel", ""), ("kernel_batched", "_batched"))}
    if workload == "selective":
        import time_selective as t
        out = {}
        for N in t.SIZES:
            res = t.time_size(N)
            for part, suffix in (("kernel", ""), ("kernel_batched", "_batched")):
                out.update({f"selective_{k}_{N}{suffix}": v["median_us"] for k, v in res[part].items()})
        return out
    if workload == "prior_shift":
        import time_prior_shift as t
        res = t.measure()
        return {f"{k}_{t.N}x{t.V}": res[k]["median_us"] for k in ("fit_priors_early_stop", "fit_priors_to_the_cap", "shift_logp")}
    if workload == "calibration":
        import time_calibration as t
        return {f"{k}_{N}x{V}": t.time_shape(N, V)[k]["median_us"] for N, V in t.SHAPES for k in ("fit_temperature",)}
    if workload == "bias_calibration":
        import time_bias_calibration as t
        return {f"fit_bias_temperature_{N}x{V}": t.time_shape(N, V)["fit_bias_temperature"]["median_us"] for N, V in t.SHAPES}
    if workload == "label_audit":
        import time_label_audit as t
        out = {}
        for N in t.SIZES:
            res = t.time_size(N)
            out.update({f"label_audit_{k}_{N}x{t.V}": res[k]["median_us"] for k in ("kernel", "kernel_batched", "joint_stages")})
        out.update({k: v["median_us"] for k, v in t.time_scatter().items() if isinstance(v, dict)})
        return out
    if workload == "epoch_scoring":
        import time_epoch_scoring as t
        from slnlp.data import synthetic_dataset
        ds = synthetic_dataset(t.ROWS, seq_len=12, src_vocab=64, n_labels=t.CLASSES, seed=6, min_len=3)
        return {f"end_epoch_{name}": 1e3 * t.time_case(ds, k, scoring)["after"]["median_ms"]
                for name, k, scoring in (("lockstep15_five_names", 15, t.FIVE), ("solo_macro_names", 1, t.MACRO))}
    from slnlp import ops
    from time_error_analysis import make_logp, timed
    zs = [make_logp(4000, 202, 1 + k)[0] for k in range(5)]
    dst = torch.empty(4000, 202, dtype=torch.float32, device="cuda")
    out = {}
    for voting in ("soft", "log"):
        fn = lambda: ops.ensemble_rows(zs, voting=voting, diagnostics=True, out=dst)
        out[f"ensemble_rows_{voting}_4000x202_k5"] = statistics.median([timed(fn) for _ in range(5 + 50)][5:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--workloads", nargs="+", choices=WORKLOADS, default=list(WORKLOADS))
    ap.add_argument("--child", choices=WORKLOADS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child)))
        return 0
    us = {}
    for r in range(a.rounds):
        for wl in a.workloads:
            for lib in (a.variant, ""):                      # parent, new, parent, new, ...
                env = dict(os.environ)
                env.pop("SLNLP_PROBE_LIB", None)
                if lib:
                    env["SLNLP_PROBE_LIB"] = lib
                got = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", wl], env=env, capture_output=True, text=True,
                                     timeout=600)
                if got.returncode != 0:
                    sys.exit(f"ab_logp_row: {wl} with {lib or 'the product library'} failed ({got.returncode}):\n{got.stderr[-2000:]}")
                for k, v in json.loads(got.stdout.strip().splitlines()[-1]).items():
                    us.setdefault(k, {"parent": [], "new": []})["parent" if lib else "new"].append(round(v, 3))
                print(f"round {r} {wl:16s} {lib or 'new'}", flush=True)
        for s in us.values():
            s.update(parent_min=min(s["parent"]), parent_max=max(s["parent"]), parent_median=statistics.median(s["parent"]),
                     new_median=statistics.median(s["new"]))
            s["new_median_within_parent_spread"] = s["parent_min"] <= s["new_median"] <= s["parent_max"]
        if a.out:                                            # after every round: a run that is cut short leaves the rounds it finished
            command = f"python tools/ab_logp_row.py --variant {a.variant} --rounds {a.rounds} --workloads {' '.join(a.workloads)}"
            with open(a.out, "w") as f:
                json.dump({"command": command, "rounds": r + 1,
                           "unit": "us: the median of one fresh process's samples, per round", "figures": us}, f, indent=1)
                f.write("\n")
    for k, s in us.items():
        print(f"{k:44s} parent {s['parent_min']:9.2f} .. {s['parent_max']:9.2f} (median {s['parent_median']:9.2f})   new median {s['new_median']:9.2f}"
              f"   {'within' if s['new_median_within_parent_spread'] else 'below' if s['new_median'] < s['parent_min'] else 'ABOVE'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
