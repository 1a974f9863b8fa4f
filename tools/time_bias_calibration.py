"""Cost of bias-corrected temperature calibration on the device (``calibration={"method": "bias_temperature"}``:
``slnlp_fit_bias_temperature``) next to ``slnlp_fit_temperature``'s 72 launches and next to the one thing a fit's calibration answers
to: one valid pass of a cfg2 fit over the same rows, on the same box.

    python tools/time_bias_calibration.py --out profiles/bias_calibration_timing.json
    rocprofv3 --kernel-trace --output-format csv -d <dir>/n800 -- python tools/time_bias_calibration.py --once 800
    rocprofv3 --kernel-trace --output-format csv -d <dir>/n4000 -- python tools/time_bias_calibration.py --once 4000
    python tools/time_bias_calibration.py --merge-trace <dir> --out profiles/bias_calibration_timing.json

Two shapes, V = 202: N = 800 (a cfg2 fit's valid split: 4000 rows split 5 ways) and N = 4000.  Per shape, on one stream of one
process, after 3 warm-up rounds, 12 rounds of: the whole fixed launch sequence of ``fit_bias_temperature`` (241 launches: the ones
behind the stop return at once), the whole sequence of ``fit_temperature`` (72), and one eval pass of the cfg2 Transformer (E 512,
8 heads, 6 layers, hidden 512, length 48, batch 50) over N rows -- ``NeuralNetClassifier._run_epoch`` -- each between two HIP events,
the second one waited for; the three alternate round by round.  The log-probs are tests/bias_calibration_ref.py's: a model trained
under uniform priors judged on long-tailed labels.  How many evaluations, halvings and Newton directions the search took is
recorded, since that is what the time buys.

The Hessian launch alone cannot be bracketed from outside the call, so it comes from a kernel trace taken in a run of its own
(``--once N``: one warm-up fit and one more, nothing else on the device): ``--merge-trace`` reads the dispatches of the fit's five
kernels from the trace and adds, per shape, the durations of the Hessian launches that did work (the longest ones, as many as
there were Newton directions) and of the other four kernels' working launches.  No pass / fail: the numbers are recorded."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

SHAPES = ((800, 202), (4000, 202))
SAMPLES, WARMUP = 12, 3
BIAS_SD = 2.0
CFG2 = dict(module__embedding_size=512, module__num_heads=8, module__num_layers=6, module__hidden_size=512)
SEQ_LEN, BATCH = 48, 50
KERNELS = ("bias_rows_kernel", "bias_classes_kernel", "bias_decide_kernel", "bias_hessian_kernel", "bias_solve_kernel")


def stats(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "min_us": float(v.min()), "max_us": float(v.max())}


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def inputs(N, V):
    import torch
    from bias_calibration_ref import make_shifted_logp
    logp, y = make_shifted_logp(N, V, 1)
    return torch.from_numpy(logp).cuda(), torch.from_numpy(y).cuda()


def search_counts(state):
    q = state.cpu().numpy().view("int64")[8:]
    return {"evaluations": int(q[1]), "halvings": int(q[5]), "newton_directions": int(q[6])}


def time_shape(N, V):
    import torch
    from slnlp import ops
    from slnlp.data import synthetic_dataset
    from slnlp.net import NeuralNetClassifier
    ds = synthetic_dataset(N, seq_len=SEQ_LEN, src_vocab=3000, n_labels=V - 2, seed=1)
    net = NeuralNetClassifier(module="model.Transformer", module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y,
                              module__batch_first=True, **CFG2, criterion__ignore_index=1, optimizer__momentum=0.9, lr=0.01,
                              batch_size=BATCH)
    torch.manual_seed(1)
    net.initialize()
    net.module_.eval()
    logp, y = inputs(N, V)
    torch.cuda.synchronize()                             # the inputs are in place before the fit's stream reads them
    us = {"fit_bias_temperature": [], "fit_temperature": [], "cfg2_valid_pass": []}
    with torch.cuda.stream(net._stream):
        X, L, yd = net._device_data(ds)
        state, bias = ops.fit_bias_temperature(logp, y, bias_sd=BIAS_SD)
        scratch = torch.empty(ops.load().slnlp_fit_bias_temperature_scratch_bytes(N, V) // 8, dtype=torch.float64, device="cuda")
        tstate = torch.empty(ops.CAL_STATE_DOUBLES, dtype=torch.float64, device="cuda")
        tscratch = torch.empty(4 * N, dtype=torch.float64, device="cuda")
        calls = {"fit_bias_temperature": lambda: ops.fit_bias_temperature(logp, y, bias_sd=BIAS_SD, state=state, bias=bias, scratch=scratch),
                 "fit_temperature": lambda: ops.fit_temperature(logp, y, state=tstate, scratch=tscratch),
                 "cfg2_valid_pass": lambda: net._run_epoch(X, L, yd, BATCH, False, 0.9, 0.5)}
        for r in range(WARMUP + SAMPLES):
            for name, fn in calls.items():
                t = timed(fn)
                if r >= WARMUP:
                    us[name].append(t)
        fit = ops.bias_temperature_download(state, bias, BIAS_SD)
        fit.pop("bias")
        fit.update(search_counts(state))
        temperature = ops.temperature_download(tstate)
    res = {"N": N, "V": V, "fit": fit, "temperature_fit": temperature, **{k: stats(v) for k, v in us.items()}}
    res["bias_fit_over_temperature_fit"] = res["fit_bias_temperature"]["median_us"] / res["fit_temperature"]["median_us"]
    res["bias_fit_over_valid_pass"] = res["fit_bias_temperature"]["median_us"] / res["cfg2_valid_pass"]["median_us"]
    res["hessian_launch"] = "not measured (needs --merge-trace)"
    return res


def once(N):
    """One warm-up fit and one more, for a kernel trace."""
    import torch
    from slnlp import ops
    logp, y = inputs(N, 202)
    for _ in range(2):
        state, bias = ops.fit_bias_temperature(logp, y, bias_sd=BIAS_SD)
        torch.cuda.synchronize()
    print(json.dumps({"N": N, **search_counts(state)}))


def merge_trace(directory, out):
    with open(out) as f:
        res = json.load(f)
    for shape in res["shapes"]:
        files = glob.glob(os.path.join(directory, f"n{shape['N']}", "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise SystemExit(f"no kernel trace under {directory}/n{shape['N']}")
        rows = [r for f in files for r in csv.DictReader(open(f))]
        newton = shape["fit"]["newton_directions"]
        evals = shape["fit"]["evaluations"]
        per = {}
        for k in KERNELS:
            d = sorted(((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]), reverse=True)
            # the trace holds two fits (the warm-up and one more): the launches that did work are the longest 2 x (how many worked)
            worked = 2 * (newton if k == "bias_hessian_kernel" else evals - 1 if k == "bias_solve_kernel" else evals + 1)
            worked = min(worked, len(d))
            per[k] = {"dispatches": len(d), "working_dispatches": worked, "working": stats(d[:worked]) if worked else None,
                      "returning_at_once": stats(d[worked:]) if len(d) > worked else None}
        shape["hessian_launch"] = per["bias_hessian_kernel"]["working"]
        shape["kernel_trace"] = per
    res["kernel_trace_command"] = "rocprofv3 --kernel-trace --output-format csv -d <dir>/n<N> -- python tools/time_bias_calibration.py --once <N>"
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({s["N"]: s["hessian_launch"] for s in res["shapes"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", type=int, default=None, help="one warm-up fit and one more at N rows, for a kernel trace")
    ap.add_argument("--merge-trace", default=None, help="directory holding n<N>/ kernel traces: add the kernels' durations to --out")
    args = ap.parse_args()
    if args.merge_trace:
        if not args.out:
            raise SystemExit("--merge-trace needs --out, the file to add to")
        return merge_trace(args.merge_trace, args.out)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_bias_calibration.py: no GPU -- nothing is measured without one")
    if args.once is not None:
        return once(args.once)
    res = {"command": "python tools/time_bias_calibration.py --out profiles/bias_calibration_timing.json", "device": torch.cuda.get_device_name(0),
           "samples": SAMPLES, "warmup": WARMUP, "bias_sd": BIAS_SD, "shapes": [time_shape(N, V) for N, V in SHAPES],
           "note": "each sample: HIP events around one call on the fit's stream, the second event waited for; the three calls alternate "
                   "round by round.  fit_bias_temperature is the whole 241-launch sequence and fit_temperature the whole 72-launch one "
                   "(the launches behind the stop return at once); cfg2_valid_pass is NeuralNetClassifier._run_epoch in eval mode over N "
                   "rows in batches of 50 (it ends with the epoch's one loss download)"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
