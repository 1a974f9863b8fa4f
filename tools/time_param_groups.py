"""Grouped vs one-group update kernels on the cfg2 module's arena (E512, 6 layers), alternated A B A B in one process:
12 samples of 20 steps each per kernel, HIP events around the 20 steps.  Writes the record profiles/param_groups_update_timing.json
was made from:  python tools/time_param_groups.py [OUT.json]"""
import json, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sign-language-nlp_amd")]
import torch
from slnlp import ops, param_groups as pg, tf_engine as te

cfg = te.make_config(512, 8, 6, 512, 3000, 202, 50, 48)
entries, n = te.layout(cfg)
pairs = [("*norm*", {"weight_decay": 0.0}), ("*bias", {"weight_decay": 0.0}), ("*embedding.weight", {"lr": 1e-4})]
groups = pg.build([e[0] for e in entries], pairs)
begin, group = pg.segments(groups, entries, n)
wd = pg.resolved(groups, {"weight_decay": 1e-2}, "weight_decay")
lrs = pg.resolved(groups, {"lr": 3e-3}, "lr")
table = ops.ParamGroupTable(n, begin, group, wd)
dev = "cuda"
g = torch.randn(n, device=dev) * 1e-3
lr1, lrG = torch.tensor([3e-3], device=dev), torch.tensor(lrs, device=dev)

def state():
    return dict(P=torch.randn(n, device=dev), M=torch.zeros(n, device=dev), V=torch.zeros(n, device=dev), c=torch.zeros(1, device=dev))
A, B = state(), state()
runs = {
    "adamw": lambda: ops.clip_adamw_step(A["P"], g, A["M"], A["V"], lr1, A["c"], weight_decay=1e-2),
    "adamw_groups": lambda: ops.clip_adam_step_groups(B["P"], g, B["M"], B["V"], table, lrG, B["c"], decoupled=True),
    "sgd": lambda: ops.clip_sgd_step_ex(A["P"], g, A["M"], lr1, A["c"], momentum=0.9, weight_decay=1e-2),
    "sgd_groups": lambda: ops.clip_sgd_step_groups(B["P"], g, B["M"], table, lrG, B["c"], momentum=0.9),
}
def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per clip + update (sumsq + update launches)
for fn in runs.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
out = {"what": "clip + update on the cfg2 arena, one-group kernels vs grouped kernels with the AdamW recipe's table (no decay on norms and biases, slower embeddings), alternated in one process", "device": "1x MI355X", "arena_floats": n, "segments": len(begin), "groups": len(groups), "unit": "us per step (sumsq + update), 20 steps per sample", "samples": {}}
for pair in (("adamw", "adamw_groups"), ("sgd", "sgd_groups")):
    s = {k: [] for k in pair}
    for rnd in range(12):                              # A B A B ...
        for k in pair:
            s[k].append(timed(runs[k]))
    for k in pair:
        out["samples"][k] = {"median": statistics.median(s[k]), "min": min(s[k]), "max": max(s[k]), "all": [round(v, 2) for v in s[k]]}
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "param_groups_update_timing.json")
json.dump(out, open(dest, "w"), indent=1)
print(json.dumps({k: {a: round(b, 2) for a, b in v.items() if a != "all"} for k, v in out["samples"].items()}), out["segments"], out["groups"], n)
