"""Cost of the training dynamics on the device (``slnlp_train_dynamics_epoch``: ``NeuralNetClassifier(train_dynamics=True)``).

    python tools/time_train_dynamics.py [--parent-tree DIR] [--out profiles/train_dynamics_timing.json]

Part 1, the update alone, in one process on one stream, at three shapes of V = 202 classes: the grid's epoch in dataset order
(N = n_visit = 4000), the same N under a balanced-style order (12000 visits drawn with repeats, so visits to one row collide), and
N = n_visit = 16384:

* ``update``: one ``ops.train_dynamics_epoch`` call -- its two launches -- between two HIP events, the second one waited for, into
  buffers allocated once; 5 warm-up calls, 50 samples; and ``update_batched``: 50 calls between one pair of events, divided by 50
  (the launch overhead a lone call pays is spread);
* ``device_route``: wall clock, between two device synchronisations, of what a fit pays per epoch -- the queued update -- plus the
  one download a report takes at the END of a fit (so a fit of E epochs pays the update E times and the download once);
* ``host_route``: wall clock of the only route to the same integers without the kernels: download the epoch's [n_visit, V]
  log-probs, then the numpy restatement (tests/train_dynamics_ref.py).  It alternates with ``device_route``, repeat by repeat
  (3 warm-up, 10 samples);
* ``same_integers``: whether both routes, started from a zeroed state, end in the same state (q may differ by one unit per
  visit where numpy's ``exp`` and the device's differ by an ulp: the count of such visits is recorded, everything else is exact).

Part 2, a fit: one train epoch (with its valid pass and epoch bookkeeping) of the cfg3 GRU (bench.py: cfg3gru -- embedding 512,
hidden 512, 4 layers, batch 50, 48 positions, 200 labels) on 4000 train rows, as wall clock of a one-epoch ``partial_fit``
(2 warm-up, 6 samples), each variant in a fresh child process: ``on``, ``off``, and -- with ``--parent-tree DIR``, a built checkout
of the parent commit -- the identical part of THIS script on that tree, twice (``parent``, ``parent_again``: their difference is
the run-to-run spread).  The script passes ``train_dynamics`` only where the estimator accepts it, so it runs on the parent
unchanged.  No pass / fail: the numbers are recorded."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.abspath(__file__)


def tree_argument(argv):
    for i, a in enumerate(argv):
        if a == "--tree" and i + 1 < len(argv):
            return os.path.abspath(argv[i + 1])
    return None


ROOT = tree_argument(sys.argv) or os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

V = 202
SHAPES = (("dataset_order_4000", 4000, 4000, False), ("balanced_style_4000x3", 4000, 12000, True), ("dataset_order_16384", 16384, 16384, False))
KERNEL_WARMUP, KERNEL_SAMPLES, ROUTE_WARMUP, ROUTE_SAMPLES = 5, 50, 3, 10
CFG = dict(E=512, Hd=512, layers=4, Vs=3000, labels=200, B=50, S=48, rows=5000)
EPOCH_WARMUP, EPOCH_SAMPLES = 2, 6


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


def make_epoch(N, n, repeats, seed):
    """log-softmax of ``3 randn`` logits with the true class raised by 4 (so some visits are wrong), labels by row, and the order"""
    g = torch.Generator().manual_seed(seed)
    order = torch.randint(0, N, (n,), generator=g) if repeats else None
    rows = order if repeats else torch.arange(n)
    y = (rows * 7 + 3) % V
    logits = 3.0 * torch.randn(n, V, generator=g, dtype=torch.float64)
    logits[torch.arange(n), y] += 4.0
    return torch.log_softmax(logits, dim=1).float().cuda(), y.cuda(), (None if order is None else order.cuda())


def time_shape(name, N, n, repeats):
    import train_dynamics_ref as R
    from slnlp import ops
    print(f"[time_train_dynamics] {name} ...", file=sys.stderr, flush=True)
    logp, y, order = make_epoch(N, n, repeats, 1)
    y_host, order_host = y.cpu().numpy(), (None if order is None else order.cpu().numpy())
    buf = ops.train_dynamics_reset(ops.train_dynamics_buffers(N, n, "cuda"))
    epoch = [0]

    def update():
        epoch[0] += 1
        ops.train_dynamics_epoch(logp, y, order, epoch[0], buf)
    update()
    torch.cuda.synchronize()
    lone = stats([timed_us(update) for _ in range(KERNEL_WARMUP + KERNEL_SAMPLES)][KERNEL_WARMUP:], "us")
    batched = stats([timed_us(update, KERNEL_SAMPLES) for _ in range(3 + 10)][3:], "us")
    host_state = [R.new_state(N)]

    def device_route():
        update()
        return ops.train_dynamics_download(buf)

    def host_route():
        return R.epoch_ref(host_state[0], logp.cpu().numpy(), y_host, order_host, 1)[0]
    routes = {"device_route": device_route, "host_route": host_route}
    ms = {k: [] for k in routes}
    for r in range(ROUTE_WARMUP + ROUTE_SAMPLES):
        for which in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
            dt, _ = wall_ms(routes[which])
            if r >= ROUTE_WARMUP:
                ms[which].append(dt)
    # both routes once more from a zeroed state: the same integers?
    ops.train_dynamics_reset(buf)
    ops.train_dynamics_epoch(logp, y, order, 1, buf)
    got = ops.train_dynamics_download(buf, per_visit=True)
    want, vis = R.epoch_ref(R.new_state(N), logp.cpu().numpy(), y_host, order_host, 1)
    exact = all(np.array_equal(np.asarray(got[k]).astype(np.int64), want[k]) for k in ("sum_mq", "head") + R.ROW_INTS)
    gap = np.abs(got["q"] - vis["q"])
    res = {"name": name, "N": N, "n_visit": n, "V": V, "order": "with repeats" if repeats else None, "update": lone, "update_batched": batched,
           **{k: stats(v, "ms") for k, v in ms.items()},
           "same_integers": {"everything_but_q": bool(exact), "mq_equal": bool(np.array_equal(got["mq"], vis["mq"])),
                             "q_visits_differing_by_one_unit": int((gap == 1).sum()), "q_visits_differing_by_more": int((gap > 1).sum()),
                             "sum_q_equal": bool(np.array_equal(got["sum_q"], want["sum_q"]))},
           "logp_bytes_per_epoch": int(n * V * 4), "report_download_bytes": int(buf["packed"].at["last"][3])}
    res["host_over_device"] = res["host_route"]["median_ms"] / res["device_route"]["median_ms"]
    return res


def epoch_part():
    """One-epoch ``partial_fit`` calls of the cfg3 GRU: {"on": ..., "off": ...} where the estimator takes the option, else {"off": ...}"""
    import inspect

    from slnlp.data import synthetic_dataset
    from slnlp.net import NeuralNetClassifier
    ds = synthetic_dataset(CFG["rows"], seq_len=CFG["S"], src_vocab=CFG["Vs"], n_labels=CFG["labels"], seed=1, min_len=8)
    takes = "train_dynamics" in inspect.signature(NeuralNetClassifier.__init__).parameters
    out = {"accepts_option": takes, "train_rows": None}
    for mode in (("off", "on") if takes else ("off",)):
        kw = {"train_dynamics": mode == "on"} if takes else {}
        net = NeuralNetClassifier(module="model.EncoderDecoderGRUAttn", module__embedding_size=CFG["E"], module__hidden_size=CFG["Hd"],
                                  module__num_layers=CFG["layers"], module__dropout=0.1, module__src_vocab=ds.vocab_X,
                                  module__tgt_vocab=ds.vocab_y, module__batch_first=True, criterion="torch.nn.CrossEntropyLoss",
                                  criterion__ignore_index=1, optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05, max_epochs=1,
                                  batch_size=CFG["B"], device="cuda", gradient_clipping={"gradient_clip_value": 0.5}, **kw)
        torch.manual_seed(1)
        net.initialize()
        ms = [wall_ms(lambda: net.partial_fit(ds))[0] for _ in range(EPOCH_WARMUP + EPOCH_SAMPLES)][EPOCH_WARMUP:]
        out[mode] = dict(stats(ms, "ms"), samples=EPOCH_SAMPLES, last_train_loss=float(net.history[-1]["train_loss"]))
        out["train_rows"] = int(len(net._train_split(ds)[0]))
        if mode == "on":
            res = net.train_dynamics()
            out["on"]["report"] = {k: res[k] for k in ("rows", "rows_seen", "epochs", "visits", "never_learned_rows", "forgetting_events")}
    return out


def child(tree, tag):
    """This script's epoch part on ``tree`` (None: this one) in a fresh process; its JSON"""
    print(f"[time_train_dynamics] the {tag} epoch part ...", file=sys.stderr, flush=True)
    cmd = [sys.executable, HERE, "--part", "epoch"] + (["--tree", tree] if tree else [])
    done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
    if done.returncode != 0:
        raise SystemExit(f"tools/time_train_dynamics.py: the {tag} epoch part ended with status {done.returncode}")
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", default="all", choices=("all", "update", "epoch"))
    ap.add_argument("--tree", default=None, help="run on this tree's package instead of the script's own (the epoch part on a parent checkout)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its epoch is timed twice beside this tree's")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_train_dynamics.py: no GPU -- nothing is measured without one")
    if args.part == "epoch":
        print(json.dumps(epoch_part()))
        return
    res = {"command": "python tools/time_train_dynamics.py --parent-tree <checkout of the parent commit> --out profiles/train_dynamics_timing.json",
           "device": torch.cuda.get_device_name(0), "shapes": [time_shape(*s) for s in SHAPES]}
    if args.part == "all":
        here = child(None, "own")
        fit = {"model": "cfg3gru", **{k: CFG[k] for k in ("E", "Hd", "layers", "B", "S", "labels")}, "train_rows": here["train_rows"],
               "on": here["on"], "off": here["off"]}
        if args.parent_tree:
            first, again = child(args.parent_tree, "parent"), child(args.parent_tree, "parent again")
            assert not first["accepts_option"], "--parent-tree: that tree's estimator takes train_dynamics, it is no parent of this change"
            fit.update(parent=first["off"], parent_again=again["off"])
            p, q = first["off"]["median_ms"], again["off"]["median_ms"]
            spread = abs(p - q)
            base = 0.5 * (p + q)
            fit["parent_run_to_run_spread_ms"] = spread
            fit["on_over_parent_ms"] = fit["on"]["median_ms"] - base
            fit["on_over_parent_percent"] = 100.0 * (fit["on"]["median_ms"] - base) / base
            fit["off_minus_parent_ms"] = fit["off"]["median_ms"] - base
            fit["off_within_parent_spread"] = bool(min(p, q) <= fit["off"]["median_ms"] <= max(p, q)
                                                   or abs(fit["off"]["median_ms"] - base) <= spread)
        res["fit_epoch"] = fit
    res["note"] = ("update: HIP events around one ops.train_dynamics_epoch call (two launches), the second event waited for; update_batched: "
                   "50 calls between one pair of events, per call; device_route / host_route: wall clock between two device "
                   "synchronisations, alternating, of the update + the report's one download, and of logp.cpu() + the numpy restatement; "
                   "fit_epoch: wall clock of a one-epoch partial_fit (train pass, valid pass, epoch bookkeeping) in fresh child processes, "
                   "medians of 6 after 2 warm-up; parent / parent_again: the same script part on a checkout of the parent commit, twice")
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
