#!/usr/bin/env python3
"""CRC-32 of every output of the kernels that share csrc/logp_row.hpp, on small inputs chosen where a row head can go wrong --
"same bits as another build" for the log-prob judging kernels, as tools/step_bits.py is for the train step.

    python tools/logp_bits.py                          one JSON line per call, of the product library
    SLNLP_PROBE_LIB=parent python tools/logp_bits.py   the same of lib/libslnlp_probeparent.so (make VARIANT=parent in the old tree)
    python tools/logp_bits.py --compare parent [--out profiles/logp_row_bits.json]
        one fresh child process per library, the lines compared; exit status 1 if any differs

Ops: reliability_rows, topk_rows, conformal_rows (scores only; LAC with threshold and set words; randomised APS with lam > 0 and
set words), ensemble_rows (soft and log, K = 1 and K = 3, with diagnostics) and, as controls that do not use the header,
scale_logp and score_rows.  Each at beta absent, beta = 1 and beta = 1 / 6 (where the op takes one), for V in {1, 63, 64, 65, 202}
and N in {1, 5, 37}, rows padded to a stride of V + 3.  Row i of a matrix is of kind (i + the index of V) mod 6: two columns tied at
the maximum, all V tied, -inf columns, a NaN, a maximum of +inf, plain -- so that N = 1 meets every special kind once over the five
V; its label is 0, V - 1, -1, V or a random class by the same rule mod 5.

On the same grid, the kernels that share csrc/block_reduce.hpp and csrc/rank_chunk.hpp: ranking_rows (rows and table) and
fit_temperature (state) where beta is absent; selective_rows for each of the three scores with and without a threshold,
selective_counts with two risk and two coverage levels (counts and table), conformal_quantile (state) and fit_priors (table and
state, 5 iterations) at every beta.  Then ranking_rows and selective_counts alone at N = 2049 and N = 4133 with V = 3
(make_chunked): more members than one LDS chunk of 2048 holds, ties across the chunk boundaries.
"""
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd")):
    sys.path.insert(0, p)

VS, NS, BETAS = (1, 63, 64, 65, 202), (1, 5, 37), (None, 1.0, 1.0 / 6.0)
CHUNK_NS = (2049, 4133)                                      # ranking_rows and selective_counts across their chunks of 2048
LEVELS = ((0.1, 0.3), (0.5, 0.9))                            # selective_counts: risks, coverages


def make(torch, N, V, vi, seed):
    """-> (logp float32 [N, V] with row stride V + 3, y int64 [N]) on the host"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * V + N)
    z = torch.log_softmax(4.0 * torch.randn(N, V, generator=g, dtype=torch.float64), dim=1).float()
    y = torch.randint(0, V, (N,), generator=g)
    inf = float("inf")
    for i in range(N):
        kind, a, b = (i + vi) % 6, (3 * i) % V, (3 * i + V // 2 + 1) % V
        if kind == 0:
            z[i, a] = z[i, b] = z[i].max() + 0.5
        elif kind == 1:
            z[i] = z[i, 0]
        elif kind == 2:
            z[i, a] = -inf
            z[i, V - 1] = -inf                               # (V = 1: the whole row, a maximum of -inf)
        elif kind == 3:
            z[i, b] = float("nan")
        elif kind == 4:
            z[i, a] = inf
        y[i] = (0, V - 1, -1, V, int(y[i]))[(i + vi) % 5]
    pad = torch.full((N, V + 3), 7.0)
    pad[:, :V] = z
    return pad, y


def make_chunked(torch, N):
    """-> (logp float32 [N, 3] with row stride 6, y int64 [N], kappa float64 [N], rows int32 [N, 4]) on the host: inputs whose
    members fill more than one LDS chunk of 2048.  Every value is one of 17, -0.0 and +0.0 among them, so ties span the chunk
    boundaries.  N = 2049: every row is a positive of class 0 and an included row (one member beyond the boundary leaves room
    for no other kind).  Larger N: 5 labels out of range, 20 rows of the other two classes, and NaNs in 4 rows -- a kappa, and
    column 1 of the matrix (class 1 is undefined; class 0 stays ranked over more than two chunks) -- at random rows, and one row
    of class 1 and one label out of range right at the first chunk boundary (rows 2047 and 2050)."""
    g = torch.Generator().manual_seed(77 + N)
    vals = torch.tensor([-0.0, 0.0] + [-0.125 * k for k in range(1, 16)], dtype=torch.float64)
    z = torch.full((N, 6), 7.0)
    z[:, :3] = vals[torch.randint(0, 17, (N, 3), generator=g)].float()
    kappa = vals[torch.randint(0, 17, (N,), generator=g)].clone()
    y = torch.zeros(N, dtype=torch.int64)
    rows = torch.zeros(N, 4, dtype=torch.int32)
    rows[:, 0] = torch.randint(0, 3, (N,), generator=g).int()
    rows[:, 1] = (torch.rand(N, generator=g) < 0.3).int()
    if N > 2049:
        at = torch.randperm(N, generator=g)[:29]
        y[at[:5]] = torch.tensor([-1, 3, 4, -7, 1 << 40])
        rows[at[:5], 3] = -1
        y[at[5:25]] = 1 + (torch.arange(20) & 1)
        y[2047], y[2050], rows[2050, 3] = 1, -1, -1          # a row of class 1 and a label out of range at the first chunk boundary
        nan_at = at[[23, 25, 26, 27]]                        # at[23] is a row of class 1: a positive whose own value is a NaN
        z[nan_at, 1] = float("nan")
        kappa[nan_at] = float("nan")
    return z, y, kappa, rows


def crc(*tensors):
    c = 0
    for t in tensors:
        c = zlib.crc32(t.detach().cpu().contiguous().numpy().tobytes(), c)
    return c


def lines():
    import torch
    from slnlp import ops
    dev = torch.device("cuda", 0)
    for vi, V in enumerate(VS):
        for N in NS:
            mats = [make(torch, N, V, vi, s) for s in (1, 2, 3)]
            zs = [m[0].to(dev)[:, :V] for m in mats]         # views: the stride stays V + 3
            z, y = zs[0], mats[0][1].to(dev)
            for beta in BETAS:
                state = None if beta is None else ops.temperature_state(beta, dev)
                out = {}
                out["reliability_rows"] = crc(*ops.reliability_rows(z, y, bins=15, state=state))
                out["topk_rows"] = crc(*ops.topk_rows(z, min(V, 7), state=state))
                qhat = torch.tensor([0.8, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev)
                for name, kw in (("conformal_scores", dict(method="aps", randomized=False)),
                                 ("conformal_lac_sets", dict(method="lac", qhat=qhat)),
                                 ("conformal_raps_sets", dict(method="aps", randomized=True, lam=0.01, k_reg=2, seed=3, draw=1, qhat=qhat))):
                    buf = ops.conformal_rows(z, y, state=state, **kw)
                    out[name] = crc(buf["score"], buf["rows"], *([buf["sets"]] if "qhat" in kw else []))
                for K in (1, 3):
                    for voting in ("soft", "log"):
                        got = ops.ensemble_rows(zs[:K], states=None if state is None else [state] * K, weights=(None, [3.0, 1.0, 2.0])[K // 3],
                                                voting=voting, diagnostics=True)
                        out[f"ensemble_{voting}_k{K}"] = crc(*got)
                if state is not None:
                    out["scale_logp"] = crc(ops.scale_logp(z, state))
                else:
                    out["score_rows"] = crc(*ops.score_rows(z, y))
                    out["ranking_rows"] = crc(*ops.ranking_rows(z, y))
                    out["fit_temperature"] = crc(ops.fit_temperature(z, y))
                tau = torch.tensor([0.4, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev)
                for score in ("max_prob", "margin", "neg_entropy"):
                    for name, t in ((score, None), (score + "_tau", tau)):
                        sel = ops.selective_rows(z, y, score=score, state=state, tau=t)
                        out["selective_" + name] = crc(sel["kappa"], sel["rows"])
                sel = ops.selective_rows(z, y, score="max_prob", state=state)
                out["selective_counts"] = crc(ops.selective_counts(sel, risks=LEVELS[0], coverages=LEVELS[1]), sel["counts"])
                buf = ops.conformal_rows(z, y, state=state, method="aps", randomized=False)
                out["conformal_quantile"] = crc(ops.conformal_quantile(buf, 0.1))
                source = torch.log_softmax(torch.arange(V, dtype=torch.float64, device=dev) / V, dim=0)
                out["fit_priors"] = crc(ops.fit_priors(z, source, state=state, max_iter=5))
                torch.cuda.synchronize()
                yield {"V": V, "N": N, "beta": beta, **out}
    for N in CHUNK_NS:
        z, y, kappa, rows = (t.to(dev) for t in make_chunked(torch, N))
        sel = ops.selective_buffers(N, dev)
        sel["kappa"].copy_(kappa)
        sel["rows"].copy_(rows)
        table = ops.selective_counts(sel, risks=LEVELS[0], coverages=LEVELS[1])
        out = {"ranking_rows": crc(*ops.ranking_rows(z[:, :3], y)), "selective_counts": crc(table, sel["counts"])}
        torch.cuda.synchronize()
        yield {"V": 3, "N": N, "beta": None, **out}


def compare(variant, dest):
    runs = {}
    for lib in ("", variant):                                # one fresh process per library: this one never opens the GPU
        env = dict(os.environ)
        env.pop("SLNLP_PROBE_LIB", None)
        if lib:
            env["SLNLP_PROBE_LIB"] = lib
        got = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        if got.returncode != 0:
            sys.exit(f"logp_bits: the run of {lib or 'the product library'} failed ({got.returncode}):\n{got.stderr[-2000:]}")
        runs[lib or "product"] = [json.loads(l) for l in got.stdout.splitlines() if l.startswith("{")]
    a, b = runs["product"], runs[variant]
    differing = [(x, y) for x, y in zip(a, b) if x != y]
    res = {"command": f"python tools/logp_bits.py --compare {variant}", "lines": len(a), "equal": len(a) == len(b) and not differing,
           "differing": differing, **runs}
    if dest:
        with open(dest, "w") as f:
            json.dump(res, f, indent=0)
            f.write("\n")
    print(f"logp_bits: {len(a)} lines of the product library, {len(b)} of {variant}: " + ("all equal" if res["equal"] else f"{len(differing)} DIFFER"))
    for x, y in differing[:10]:
        print("  ", {k: (x[k], y.get(k)) for k in x if x[k] != y.get(k)}, {k: x[k] for k in ("V", "N", "beta")})
    return 0 if res["equal"] else 1


def main():
    if "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
        return compare(sys.argv[i + 1], dest)
    for line in lines():
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
