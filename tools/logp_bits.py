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

The kernels that share the wave-per-row loop, the queued fits' state and the row sums (csrc/common.hpp: wave_rows, csrc/fit_state.hpp,
csrc/block_reduce.hpp) add, on the same grid: fit_bias_temperature (state and bias) where beta is absent; shift_logp out of place and
in place, label_audit_rows (a zero-filled buffer, all of it but the pairs workspace) and scatter_logp (a zero-filled target of
N + 2 rows; the row table holds -1 and N + 2 among valid targets where N >= 3) at every beta.  augment_rows and gather_batch (with and
without an order) run on id matrices of their own (make_ids).  Then ONE block at N = 8197, V = 3, stride 6 (make_wrapped) -- the
wave-per-row loop has 2048 x 4 waves, so it first wraps at row 8192, a size nothing above reaches: score_rows, reliability_rows,
topk_rows, scale_logp, shift_logp, scatter_logp, fit_temperature, fit_bias_temperature, fit_priors (max_iter 2), label_audit_rows
and ensemble_rows (K = 3).  An op that refuses its arguments puts the message in its place (the same for every build).
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


def make_wrapped(torch, N=8197):
    """-> (three logp float32 [N, 3] with row stride 6, y int64 [N]) on the host: more rows than the 8192 waves of a wave-per-row
    launch.  The special rows sit on both sides of the wrap: a NaN, a +inf maximum, a -inf column, a tie, labels out of range."""
    g = torch.Generator().manual_seed(8197)
    zs = []
    for k in range(3):
        z = torch.full((N, 6), 7.0)
        z[:, :3] = torch.log_softmax(3.0 * torch.randn(N, 3, generator=g, dtype=torch.float64), dim=1).float()
        zs.append(z)
    y = torch.randint(0, 3, (N,), generator=g)
    z = zs[0]
    for base in (3, 8190):                                   # rows 3 .. 7 and 8190 .. 8194
        z[base, 1] = float("nan")
        z[base + 1, 2] = float("inf")
        z[base + 2, 0] = -float("inf")
        z[base + 3, 0] = z[base + 3, 2] = z[base + 3].max() + 0.25
        y[base + 4] = (-1, 3)[base > 3]
    return zs, y


def make_ids(torch, n, S, seed):
    """-> (X int64 [n, S], L int64 [n], y int64 [n]) on the host: token ids, lengths in 0 .. S + 1 (one past the row: clamped), labels"""
    g = torch.Generator().manual_seed(31 * seed + 7 * n + S)
    return torch.randint(2, 900, (n, S), generator=g), torch.randint(0, S + 2, (n,), generator=g), torch.randint(0, 9, (n,), generator=g)


def attempt(fn):
    """fn()'s CRC, or the message of the ValueError / RuntimeError with which the op refused its arguments"""
    try:
        return fn()
    except (ValueError, RuntimeError) as e:
        return f"{type(e).__name__}: {e}"


def judged(torch, ops, z, y, state, fresh):
    """the ops this tool reached last: shift_logp, label_audit_rows, scatter_logp -> {name: crc}.  fresh(): a new device copy of z"""
    N, V = z.shape
    dev = z.device
    log_w = torch.log_softmax(torch.arange(V, dtype=torch.float64, device=dev) / 3.0, dim=0)
    out = {"shift_logp": attempt(lambda: crc(ops.shift_logp(z, log_w, state)))}

    def in_place():
        zc = fresh()
        ops.shift_logp(zc, log_w, state, out=zc)
        return crc(zc)
    out["shift_logp_in_place"] = attempt(in_place)

    def audit():
        buf = ops.label_audit_buffers(N, V, 5, dev)
        buf["flat"].zero_()
        ops.label_audit_rows(z, y, buf, state=state)
        return crc(buf["flat"][:buf["at"]["work"]])
    out["label_audit_rows"] = attempt(audit)

    def scatter():
        rows = torch.arange(N - 1, -1, -1, dtype=torch.int64)           # distinct targets, descending
        if N >= 3:
            rows[0], rows[N // 2] = -1, N + 2
        dst = torch.zeros(N + 2, V + 3, dtype=torch.float32, device=dev)[:, :V]
        ops.scatter_logp(z, rows.to(dev), dst, state=state)
        return crc(dst)
    out["scatter_logp"] = attempt(scatter)
    return out


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
                    out["fit_bias_temperature"] = attempt(lambda: crc(*ops.fit_bias_temperature(z, y)))
                out.update(judged(torch, ops, z, y, state, lambda: mats[0][0].to(dev)[:, :V]))
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
    for n in NS:
        for S in (1, 48, 130):
            X, L, y = (t.to(dev) for t in make_ids(torch, n, S, 5))
            order = torch.randperm(n, generator=torch.Generator().manual_seed(n)).to(dev)
            out = {f"augment_rows_{k}": crc(*ops.augment_rows(X, L, 0, 1, pd, pm, seed=11, epoch=3))
                   for k, (pd, pm) in enumerate(((0.3, 0.2), (0.0, 0.5), (0.9, 0.0)))}
            B = max(1, n - 1)
            out["gather_batch"] = crc(*ops.gather_batch(X, L, y, None, n - B, B))
            out["gather_batch_order"] = crc(*ops.gather_batch(X, L, y, order, n - B, B))
            torch.cuda.synchronize()
            yield {"n": n, "S": S, **out}
    zs, y = make_wrapped(torch)
    zs, y = [t.to(dev)[:, :3] for t in zs], y.to(dev)
    z = zs[0]
    for beta in (None, 1.0 / 6.0):
        state = None if beta is None else ops.temperature_state(beta, dev)
        out = {"reliability_rows": crc(*ops.reliability_rows(z, y, bins=15, state=state)), "topk_rows": crc(*ops.topk_rows(z, 2, state=state)),
               "ensemble_rows": crc(*ops.ensemble_rows(zs, states=None if state is None else [state] * 3, weights=[3.0, 1.0, 2.0]))}
        source = torch.log_softmax(torch.arange(3, dtype=torch.float64, device=dev) / 3, dim=0)
        out["fit_priors"] = crc(ops.fit_priors(z, source, state=state, max_iter=2))
        if state is not None:
            out["scale_logp"] = crc(ops.scale_logp(z, state))
        else:
            out["score_rows"] = crc(*ops.score_rows(z, y))
            out["fit_temperature"] = crc(ops.fit_temperature(z, y))
            out["fit_bias_temperature"] = crc(*ops.fit_bias_temperature(z, y))
        out.update(judged(torch, ops, z, y, state, lambda: make_wrapped(torch)[0][0].to(dev)[:, :3]))
        torch.cuda.synchronize()
        yield {"V": 3, "N": z.shape[0], "beta": beta, **out}
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
    refused = sorted({k for x in a for k, v in x.items() if isinstance(v, str)})
    if refused:
        print(f"logp_bits: ops that refused their arguments on some line: {', '.join(refused)}")
    for x, y in differing[:10]:
        print("  ", {k: (x[k], y.get(k)) for k in x if x[k] != y.get(k)}, {k: x[k] for k in ("V", "N", "beta", "n", "S") if k in x})
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
