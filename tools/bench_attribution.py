"""Cost of an occlusion attribution on the device (``LogProbJudge.attribute``) at the grid's epoch: 4000 rows x 202 classes, a cfg3
GRU (bench.py: cfg3gru -- embedding 512, hidden 512, 4 layers, source vocabulary 3000, 48 positions, batch 50), frame mode (every
frame of every row masked once), next to the only route to the same numbers without the kernels: build nothing on the device's
side of the reduction -- download every variant's log-probs and run the numpy restatement (tests/attribution_ref.py) with the same
report.  The forward passes are the same on both routes and are reported on their own.

    python tools/bench_attribution.py [--rows 4000] [--out profiles/attribution_timing.json]

Measurements, one process, the estimator's own stream, wall clock between device synchronisations, summed over the chunks of at most
``max_variants`` variants that ``attribute`` itself walks through:

* ``base_forward``: the base pass through the hook;
* ``builder``: ``ops.occlude_rows`` of every chunk;
* ``variant_forward``: the forward passes on the chunks' ``DeviceRows`` through the hook, their ``then`` a no-op;
* ``attribution_rows``: ``ops.attribution_rows`` of every chunk on log-probs kept from those passes;
* ``summary``: ``ops.attribution_summary``; ``download``: the ONE ``ops.attribution_download``; ``report``: ``metrics.attribution_report``;
* ``attribute``: one ``net.attribute(ds)`` call end to end;
* ``host_download``: ``.cpu()`` of every chunk's [m, V] log-probs; ``host_restatement``: ``attribution_ref`` and the same report.

The stages that take seconds (the forward passes, the restatement, ``attribute``) are sampled once after a warm-up on the first 200
rows; the sub-millisecond ones (builder, ``attribution_rows``, summary, download, report) and the host download are repeated on the
kept buffers -- 3 warm-up and 20 samples (host download: 5) -- and reported as median / min / max.  The fit is one epoch of SGD on
synthetic rows: the weights do not matter to the cost.  No pass / fail: the numbers are recorded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

CFG = dict(E=512, Hd=512, layers=4, Vs=3000, labels=200, B=50, S=48)
MAX_VARIANTS = 65536


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def repeated(fn, samples=20, warmup=3):
    v = np.asarray([wall_ms(fn)[0] for _ in range(warmup + samples)][warmup:])
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "samples": samples}


def make_net(ds):
    from slnlp.net import NeuralNetClassifier
    return NeuralNetClassifier(module="model.EncoderDecoderGRUAttn", module__embedding_size=CFG["E"], module__hidden_size=CFG["Hd"],
                               module__num_layers=CFG["layers"], module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y,
                               module__batch_first=True, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1,
                               optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05, max_epochs=1, batch_size=CFG["B"], device="cuda",
                               gradient_clipping={"gradient_clip_value": 0.5})


def stages(net, ds):
    """The steps of ``attribute`` one by one, each between two synchronisations; the chunks' log-probs are kept for the host route."""
    import attribution_ref as ar
    from slnlp import metrics, ops
    from slnlp.data import DeviceRows
    S = ds.ids.shape[1]
    ms = {}
    variants, start, nb = ops.occlusion_variants(ds.lengths, S, "mask")
    M = len(variants)
    ms["base_forward"], (base, yd) = wall_ms(lambda: net._judge(ds, lambda logp, y: (logp.clone(), y)))
    Xd, Ld = torch.from_numpy(ds.ids).cuda(), torch.from_numpy(ds.lengths).cuda()
    buf = ops.attribution_buffers(len(ds), base.shape[1], variants, start, nb, "cuda")
    chunks, first = [], 0
    while first < len(ds):
        last = first + 1
        while last < len(ds) and int(start[last + 1]) - int(start[first]) <= MAX_VARIANTS:
            last += 1
        chunks.append((int(start[first]), int(start[last]) - int(start[first])))
        first = last
    ms["variant_forward"] = 0.0
    built, kept = [], []
    for off, m in chunks:                                                        # the passes that take seconds: once
        rows = DeviceRows(*ops.occlude_rows(Xd, Ld, yd, buf["variants"][off:off + m], "mask", pad=1, unk=0))
        dt, logp = wall_ms(lambda: net._judge(rows, lambda z, y: z))
        ms["variant_forward"] += dt
        built.append(rows)
        kept.append(logp)

    def build():
        for (off, m), rows in zip(chunks, built):
            ops.occlude_rows(Xd, Ld, yd, buf["variants"][off:off + m], "mask", pad=1, unk=0, out=(rows.ids, rows.lengths, rows.y))

    def reduce_rows():
        for (off, m), logp in zip(chunks, kept):
            ops.attribution_rows(base, logp, yd, buf, off)
    ms["builder"], ms["attribution_rows"] = repeated(build), repeated(reduce_rows)
    ms["summary"] = repeated(lambda: ops.attribution_summary(base, yd, buf))
    ms["download"] = repeated(lambda: ops.attribution_download(buf))
    got = ops.attribution_download(buf)
    ms["report"] = repeated(lambda: metrics.attribution_report(got))
    dev = metrics.attribution_report(got)
    ms["host_download"] = repeated(lambda: [logp.cpu().numpy() for logp in kept], samples=5, warmup=1)
    host = [logp.cpu().numpy() for logp in kept]
    base_host, y_host = base.cpu().numpy(), np.asarray(ds.y)

    def restate():
        return metrics.attribution_report(ar.attribution_ref(base_host, np.concatenate(host), y_host, variants, start, nb, "label"))
    ms["host_restatement"], ref = wall_ms(restate)
    ms["attribute"], res = wall_ms(lambda: net.attribute(ds, max_variants=MAX_VARIANTS))
    same = {"top_unit_equal": bool(np.array_equal(dev["top_unit"], ref["top_unit"])), "flips_equal": bool(np.array_equal(dev["flips"], ref["flips"])),
            "counts_equal": bool(np.array_equal(dev["per_class"]["count"], ref["per_class"]["count"])),
            "max_mean_drop_difference": float(np.nanmax(np.abs(dev["per_bin"]["mean_drop"] - ref["per_bin"]["mean_drop"]))),
            "attribute_top_unit_equal": bool(np.array_equal(res["top_unit"], dev["top_unit"]))}
    return {"rows": len(ds), "classes": int(base.shape[1]), "variants": M, "chunks": len(chunks), "max_variants": MAX_VARIANTS,
            "variant_logp_megabytes": M * base.shape[1] * 4 / 1e6, "download_bytes": int(buf["at"]["vals"]) * 4, "ms": ms,
            "device_after_forward_ms": sum(ms[k]["median_ms"] for k in ("builder", "attribution_rows", "summary", "download", "report")),
            "host_after_forward_ms": ms["host_download"]["median_ms"] + ms["host_restatement"], "check": same,
            "mean_drop_per_bin": [float(v) for v in dev["per_bin"]["mean_drop"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_attribution.py: no GPU -- nothing is measured without one")
    from slnlp.data import synthetic_dataset
    ds = synthetic_dataset(args.rows, seq_len=CFG["S"], src_vocab=CFG["Vs"], n_labels=CFG["labels"], seed=1, min_len=8)
    torch.manual_seed(1)
    net = make_net(ds).fit(ds)
    stages(net, ds[np.arange(min(200, len(ds)))])                                # warm-up
    res = {"command": f"python tools/bench_attribution.py --rows {args.rows} --out profiles/attribution_timing.json",
           "device": torch.cuda.get_device_name(0), "config": CFG, "by": "frame", "mode": "mask", **stages(net, ds),
           "note": "wall clock between device synchronisations, summed over the chunks, after a warm-up on 200 rows: one sample of the stages that "
                   "take seconds, median / min / max of 20 samples (host_download: 5) of the others; "
                   "device_after_forward_ms = builder + attribution_rows + summary + download + report; host_after_forward_ms = the download of "
                   "every variant's log-probs + the numpy restatement with the same report; the forward passes (base_forward, variant_forward) "
                   "are common to both routes; the builder has no host counterpart here (a host route would also build and upload the variants)"}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
