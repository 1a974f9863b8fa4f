"""Cost of the reliability diagnostics on the device (``slnlp_reliability_rows``: the ``neg_ece`` / ``neg_mce`` / ``neg_brier``
scoring names, ``NeuralNetClassifier.reliability``) next to the existing pass of the same shape and to what an epoch's scoring
answers to: one valid pass of a cfg2 fit over the same rows.

    python tools/time_reliability.py [--out profiles/reliability_timing.json]

Two shapes: N = 800, V = 202 (a cfg2 fit's valid split: 4000 rows split 5 ways) and N = 3000, V = 300.  Per shape, on one stream
of one process, after 3 warm-up rounds, 12 rounds of: one ``ops.reliability_rows`` (15 bins, beta = 1 as the null pointer: what an
epoch runs), one with beta = 1 read from a state (the same arithmetic), one with beta = 1 / 6 read from a state (the same launches
on exponents six times smaller), one ``ops.score_rows`` on the same matrix, and one eval pass of the cfg2 Transformer
(E 512, 8 heads, 6 layers, hidden 512, length 48, batch 50; a V-class head) over N rows -- ``NeuralNetClassifier._run_epoch`` --
each between two HIP events, the second one waited for, all into buffers allocated once; the four small calls rotate their order
from round to round, so that none of them is always the one that follows the valid pass's host wait.  Then each small call is timed
again in a loop of its own (``back_to_back``: 3 warm-up calls, 12 samples, nothing else in between).  The log-probs are log-softmax of
``8 randn`` logits with the true class raised in 60 % of the rows.  No pass / fail: the numbers are recorded."""
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
SEQ_LEN, BATCH, BINS = 48, 50, 15


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
    us = {"reliability_rows": [], "reliability_rows_state_1": [], "reliability_rows_beta": [], "score_rows": [], "cfg2_valid_pass": []}
    with torch.cuda.stream(net._stream):
        X, L, yd = net._device_data(ds)
        state, state_1 = ops.temperature_state(1.0 / 6.0, "cuda"), ops.temperature_state(1.0, "cuda")
        rel, score = ops.reliability_buffers(N, BINS, "cuda"), ops.score_buffers(N, V, "cuda")
        calls = {"reliability_rows": lambda: ops.reliability_rows(logp, y, bins=BINS, out=rel),
                 "reliability_rows_state_1": lambda: ops.reliability_rows(logp, y, bins=BINS, state=state_1, out=rel),
                 "reliability_rows_beta": lambda: ops.reliability_rows(logp, y, bins=BINS, state=state, out=rel),
                 "score_rows": lambda: ops.score_rows(logp, y, out=score),
                 "cfg2_valid_pass": lambda: net._run_epoch(X, L, yd, BATCH, False, 0.9, 0.5)}
        small = [k for k in calls if k != "cfg2_valid_pass"]
        for r in range(WARMUP + SAMPLES):
            # the small calls take turns at every place of the round, the one behind the valid pass's host wait included
            k = r % len(small)
            for name in small[k:] + small[:k] + ["cfg2_valid_pass"]:
                t = timed(calls[name])
                if r >= WARMUP:
                    us[name].append(t)
        # ... and each small call in a loop of its own, back to back: no other kernel and no host wait between two samples
        alone = {}
        for name in small:
            alone[name] = [timed(calls[name]) for _ in range(WARMUP + SAMPLES)][WARMUP:]
        ops.reliability_rows(logp, y, bins=BINS, out=rel)
        summary = ops.reliability_download(rel)
    res = {"N": N, "V": V, "bins": BINS, "summary": {k: summary[k] for k in ("ece", "mce", "brier", "nll", "accuracy", "confidence")},
           **{k: stats(v) for k, v in us.items()}, "back_to_back": {k: stats(v) for k, v in alone.items()}}
    res["reliability_over_score_rows"] = res["reliability_rows"]["median_us"] / res["score_rows"]["median_us"]
    res["reliability_over_valid_pass"] = res["reliability_rows"]["median_us"] / res["cfg2_valid_pass"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_reliability.py: no GPU -- nothing is measured without one")
    res = {"command": "python tools/time_reliability.py --out profiles/reliability_timing.json", "device": torch.cuda.get_device_name(0),
           "samples": SAMPLES, "warmup": WARMUP, "shapes": [time_shape(N, V) for N, V in SHAPES],
           "note": "each sample: HIP events around one call on the fit's stream, the second event waited for; every round runs the five calls, the "
                   "four small ones in rotating order, the valid pass last; back_to_back: each small call again in a loop of its own.  reliability_rows is two launches (the rows, then bins + 1 blocks for the table), score_rows two "
                   "(zeroing the counts, then the rows); cfg2_valid_pass is NeuralNetClassifier._run_epoch in eval mode over N rows in batches of 50 (it ends with the "
                   "epoch's one loss download)"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
