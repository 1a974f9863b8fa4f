#!/usr/bin/env python3
"""CRC-32 of what a few train steps of ONE named case leave behind -- "same bits as another build" as a command.

    python tools/step_bits.py CASE        (--list: the case names, one per dispatch branch of the plans)
    SLNLP_PROBE_LIB=old python tools/step_bits.py CASE      the same with lib/libslnlp_probeold.so (as tools/ab_bench.py)

The case's engine(s) get slnlp/synth.py weights and a fixed synthetic batch per step; one eval forward, then the train steps.
One JSON line: the CRCs of the eval and last train log-probs, of the parameter / gradient / momentum arenas and of `scalars`
(lockstep cases: over all fits, plus the launches per step).  Runs in this process: start one fresh child per library and
compare the lines -- every CRC must be equal.
"""
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd")):
    sys.path.insert(0, p)

TF1 = dict(E=128, H=4, N=2, F=256, Vs=3000, Vt=202, B=50, S=48, dropout=0.1)
RNN3 = dict(E=512, Hd=512, N=4, Vs=3000, Vt=202, B=50, S=48, dropout=0.1)
RNN0 = dict(E=24, Hd=32, N=2, Vs=300, Vt=40, B=8, S=10, dropout=0.1)
TF0 = dict(E=32, H=4, N=2, F=64, Vs=300, Vt=40, B=8, S=12, dropout=0.1)
# name -> (config, options: steps / graph / lockstep K / adam / update (set_update's arguments) / groups (per fit: a table?) / env)
CASES = {
    "tf_tiny": (TF0, {}),                                                                        # fp32-operand path everywhere
    "tf_cfg1_d0": (dict(TF1, dropout=0.0), {}),                                                  # planes + B-row products
    "tf_cfg1": (TF1, {}),                                                                        # ... masked LayerNorm planes, per-head dropout
    "tf_cfg1_decrows0": (TF1, dict(env={"SLNLP_DEC_ROWS": "0"})),                                # plane encoder, fp32-operand decoder
    "tf_cfg1_s128": (dict(TF1, S=128), {}),                                                      # long attention, non-lean workspace
    "tf_cfg1_graph": (TF1, dict(graph=True)),                                                    # captured step
    "tf_cfg1_ls3": (TF1, dict(lockstep=3)),                                                      # recorder: pairs not deferred
    "tf_cfg2": (dict(E=512, H=8, N=6, F=512, Vs=3000, Vt=202, B=50, S=48, dropout=0.1), dict(steps=3)),   # deferred weight gradients, batched d memory
    "tf_b256": (dict(E=256, H=4, N=2, F=256, Vs=3000, Vt=202, B=256, S=16, dropout=0.1), {}),    # plane GEMM for the decoder (but the V projection)
    "tf_fp8": (dict(TF1, precision=8), {}),                                                      # fp8 forward products
    "tf_cfg1_adam": (TF1, dict(adam=True)),
    "rnn_lstm_tiny": (dict(RNN0, rnn="lstm"), {}), "rnn_gru_tiny": (dict(RNN0, rnn="gru"), {}),  # RNN fp32 path
    "rnn_lstm_cfg3_d0": (dict(RNN3, rnn="lstm", dropout=0.0), dict(steps=3)), "rnn_lstm_cfg3": (dict(RNN3, rnn="lstm"), dict(steps=3)),   # planes path
    "rnn_gru_cfg3_d0": (dict(RNN3, rnn="gru", dropout=0.0), dict(steps=3)), "rnn_gru_cfg3": (dict(RNN3, rnn="gru"), dict(steps=3)),
    "rnn_lstm_cfg3_ls3": (dict(RNN3, rnn="lstm"), dict(steps=3, lockstep=3)),                    # RNN recorder path
    # the fused update's dispatch branches (csrc/update.hip)
    "tf_tiny_sgd_damp_wd": (TF0, dict(update=dict(dampening=0.3, weight_decay=1e-2))),           # SGD's general loop
    "tf_tiny_sgd_nesterov": (TF0, dict(update=dict(nesterov=True))),
    "rnn_lstm_tiny_adamw": (dict(RNN0, rnn="lstm"), dict(adam=True, update=dict(kind="adamw", weight_decay=1e-2))),   # a skip range (the dead pre-output bias)
    "tf_tiny_groups_sgd": (TF0, dict(groups=(True,), update=dict(weight_decay=1e-2))),           # the table kernels
    "tf_tiny_groups_adamw": (TF0, dict(groups=(True,), adam=True, update=dict(kind="adamw", weight_decay=1e-2))),
    "tf_cfg1_groups": (TF1, dict(groups=(True,))),                                               # ... writing the weight planes
    "tf_tiny_ls3_groups": (TF0, dict(lockstep=3, groups=(True, True, False), update=dict(weight_decay=1e-2))),   # the ungrouped fit on a one-segment table
}


def group_table(e, f, torch):
    """One segment per arena entry, dealt over 3 groups (fit f starts at group f) with their own weight decay and rate."""
    begin = sorted({off for _, _, off in e.entries})
    table = {"seg_begin": begin, "seg_group": [(i + f) % 3 for i in range(len(begin))], "weight_decay": [1e-2, 0.0, 1e-3]}
    return table, torch.tensor([0.01 * (1 + f), 0.02, 0.005], device=e.device)


def crc(*tensors):
    c = 0
    for t in tensors:
        c = zlib.crc32(t.detach().cpu().contiguous().numpy().tobytes(), c)
    return c


def main():
    if len(sys.argv) != 2 or sys.argv[1] == "--list" or sys.argv[1] not in CASES:
        print("\n".join(CASES))
        return 0 if sys.argv[1:] == ["--list"] else 2
    c, o = CASES[sys.argv[1]]
    os.environ.update(o.get("env", {}))           # read by the library when the plan is created
    import torch
    import bench
    from slnlp import synth, tf_engine as te, rnn_engine as re_
    from slnlp.lockstep import LockstepGroup
    dev = torch.device("cuda", 0)
    rnn, steps, K, B, S = "rnn" in c, o.get("steps", 4), o.get("lockstep", 1), c["B"], c["S"]
    engs, data = [], []
    for f in range(K):                            # lockstep fits differ in weights, data, dropout rate and learning rate
        cfg, sd = bench.build_sd(dict(c, dropout=c["dropout"] * (1 + f)), seed=1 + f)
        e = (re_.RnnEngine if rnn else te.TransformerEngine)(cfg, device=dev, seed=1 + f)
        e.load_state(sd)
        e.set_lr(0.01 * (1 + f))
        if o.get("update"):
            e.set_update(**o["update"])
        if f < len(o.get("groups", ())) and o["groups"][f]:
            e.set_param_groups(*group_table(e, f, torch))
        X, L, y = (torch.from_numpy(a).to(dev) for a in synth.make_batch(steps * B, S, c["Vs"], c["Vt"], seed=1 + f))
        engs.append(e)
        data.append((X, y, L))
    out = {"case": sys.argv[1], "lib": os.environ.get("SLNLP_PROBE_LIB", "")}
    with torch.cuda.stream(torch.cuda.Stream()):
        e, (X, y, L) = engs[0], data[0]
        batch = lambda i: (X[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) + ((L[i * B:(i + 1) * B],) if rnn else ())
        out["eval_logp"] = crc(e.forward(*batch(0), train=False))
        if K > 1:
            grp = LockstepGroup(engs)
            grp.set_data(0, [d[0] for d in data], [d[1] for d in data], B, [d[2] for d in data])
            grp.epoch(0, B, True, 0.9, 0.5)
            torch.cuda.synchronize()
            out["launches"] = grp.num_launches(0, B, True)
            out["logp"] = crc(*grp.logp[0], *grp.loss[0])
            grp.close()
        else:
            v2 = torch.zeros_like(e.params) if o.get("adam") else None
            for i in range(steps):
                if v2 is not None:
                    logp = e.train_step_adam(*batch(i)[:2], v2, weight_decay=o.get("update", {}).get("weight_decay", 0.0),
                                             lengths=batch(i)[2] if rnn else None)
                else:
                    logp = (e.train_step_graph if o.get("graph") else e.train_step)(*batch(i))
            out["logp"] = crc(logp, *([v2] if v2 is not None else []))
        torch.cuda.synchronize()
    for k in ("params", "grads", "momentum", "scalars"):
        out[k] = crc(*[getattr(e, k) for e in engs])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
