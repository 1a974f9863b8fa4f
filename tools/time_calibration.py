"""Cost of temperature calibration on the device (``calibration={"method": "temperature"}``: ``slnlp_fit_temperature``,
``slnlp_scale_logp``) next to the one thing it answers to: one valid pass of a cfg2 fit over the same rows.

    python tools/time_calibration.py [--out profiles/calibration_timing.json]

Two shapes: N = 800, V = 202 (a cfg2 fit's valid split: 4000 rows split 5 ways) and N = 3000, V = 300.  Per shape, on one stream
of one process, after 3 warm-up rounds, 12 rounds of: the whole fixed launch sequence of ``fit_temperature``, one ``scale_logp``
(out of place), and one eval pass of the cfg2 Transformer (E 512, 8 heads, 6 layers, hidden 512, length 48, batch 50; a V-class
head) over N rows -- ``NeuralNetClassifier._run_epoch``, what ``partial_fit`` runs per epoch and once more to calibrate --
each between two HIP events, the second one waited for.  The log-probs that are fitted are log-softmax of ``8 randn`` logits with
the true class raised in 60 % of the rows (an overconfident model, T about 6): the iterations the search took are recorded,
since the launches behind the stop return at once.  No pass / fail: the numbers are recorded; the fit calibrates once."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

SHAPES = ((800, 202), (3000, 300))
SAMPLES, WARMUP = 12, 3
CFG2 = dict(module__embedding_size=512, module__num_heads=8, module__num_layers=6, module__hidden_size=512)
SEQ_LEN, BATCH = 48, 50


def stats(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "min_us": float(v.min()), "max_us": float(v.max())}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def overconfident_logp(N, V, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, V, (N,), generator=g)
    logits = 8.0 * torch.randn(N, V, generator=g, dtype=torch.float64)
    rows = torch.nonzero(torch.rand(N, generator=g) < 0.6).squeeze(1)
    logits[rows, y[rows]] += 32.0
    return torch.log_softmax(logits, dim=1).float().cuda(), y.cuda()


def time_shape(N, V):
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
    logp, y = overconfident_logp(N, V, 1)
    torch.cuda.synchronize()                             # the inputs are in place before the fit's stream reads them
    us = {"fit_temperature": [], "scale_logp": [], "cfg2_valid_pass": []}
    with torch.cuda.stream(net._stream):
        X, L, yd = net._device_data(ds)
        state = torch.empty(ops.CAL_STATE_DOUBLES, dtype=torch.float64, device="cuda")
        scratch = torch.empty(4 * N, dtype=torch.float64, device="cuda")
        out = torch.empty_like(logp)
        calls = {"fit_temperature": lambda: ops.fit_temperature(logp, y, state=state, scratch=scratch),
                 "scale_logp": lambda: ops.scale_logp(logp, state, out=out),
                 "cfg2_valid_pass": lambda: net._run_epoch(X, L, yd, BATCH, False, 0.9, 0.5)}
        for r in range(WARMUP + SAMPLES):
            for name, fn in calls.items():
                t = timed(fn)
                if r >= WARMUP:
                    us[name].append(t)
        fit = ops.temperature_download(state)
    res = {"N": N, "V": V, "fit": fit, **{k: stats(v) for k, v in us.items()}}
    res["fit_over_valid_pass"] = res["fit_temperature"]["median_us"] / res["cfg2_valid_pass"]["median_us"]
    res["scale_over_valid_pass"] = res["scale_logp"]["median_us"] / res["cfg2_valid_pass"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_calibration.py: no GPU -- nothing is measured without one")
    res = {"command": "python tools/time_calibration.py --out profiles/calibration_timing.json", "device": torch.cuda.get_device_name(0),
           "samples": SAMPLES, "warmup": WARMUP, "shapes": [time_shape(N, V) for N, V in SHAPES],
           "note": "each sample: HIP events around one call on the fit's stream, the second event waited for; the three calls alternate "
                   "round by round.  fit_temperature is the whole 72-launch sequence (the launches behind the stop return at once); "
                   "cfg2_valid_pass is NeuralNetClassifier._run_epoch in eval mode over N rows in batches of 50 (it ends with the "
                   "epoch's one loss download)"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
