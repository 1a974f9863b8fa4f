"""What the order tables cost, measured on ONE box in interleaved rounds (as tools/ab_bench.py: devices differ by several per
cent, so numbers of two sessions are never compared): this tree against a built checkout of the commit before the feature.

    python tools/ab_shuffle.py --old-root DIR [--rounds 3] [--out profiles/r07_shuffle_ab.json]

  (a) bench.py ms_per_step                              this tree vs DIR
  (b) 15-fit cfg2 lockstep step, no order tables        this tree vs DIR      (tools/bench_lockstep.py --ks 15)
  (c) the same step with an order table on every fit    this tree             (--shuffle)
Every measurement is a fresh child process."""
import argparse, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--old-root", required=True)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_shuffle_ab.json"))
a = ap.parse_args()

BENCH = ["bench.py", "--gpus", "1", "--steps", "100", "--warmup", "20"]
LS = ["tools/bench_lockstep.py", "--workload", "cfg2", "--ks", "15", "--steps", "12"]
RUNS = [("bench_ms_per_step", "new", ROOT, BENCH), ("bench_ms_per_step", "old", a.old_root, BENCH),
        ("ls15_ms_per_step", "new", ROOT, LS), ("ls15_ms_per_step", "old", a.old_root, LS),
        ("ls15_ms_per_step", "new_order_tables", ROOT, LS + ["--shuffle"])]


def run(root, cmd):
    out = subprocess.run([sys.executable] + cmd, cwd=root, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"{cmd} in {root} failed ({out.returncode}): {out.stderr[-600:]}")     # nothing more is started
    d = json.loads(out.stdout.strip().splitlines()[-1])
    return d["results"][0]["ms_per_lockstep_step"] if "results" in d else d["ms_per_step"]


res = {}
for r in range(a.rounds):
    for what, who, root, cmd in RUNS:
        ms = run(root, cmd)
        res.setdefault(what, {}).setdefault(who, []).append(ms)
        print(f"round {r} {what:18s} {who:17s} {ms}", flush=True)
summary = {}
for what, by in res.items():
    for who, ms in by.items():
        summary[f"{what}.{who}"] = {"min": min(ms), "max": max(ms), "spread_pct": round(100 * (max(ms) - min(ms)) / min(ms), 2)}
doc = {"what": __doc__.split("\n\n")[0], "rounds": res, "summary": summary}
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(summary, indent=1))
