#!/usr/bin/env python3
"""CRC-32 of every output of the three neighbour searches on the inputs of their GPU tests -- "same bits as another build" for
csrc/edit_knn.hip, csrc/edit_long.hip and csrc/field_knn.hip, as tools/logp_bits.py is for the log-prob judging kernels.

    python tools/knn_bits.py                          one JSON line per case, of the product library
    SLNLP_PROBE_LIB=parent python tools/knn_bits.py   the same of lib/libslnlp_probeparent.so (make VARIANT=parent in the old tree)
    python tools/knn_bits.py --compare parent [--out profiles/knn_shell_bits.json]
        one fresh child process per library, each under its own time limit, the lines compared; stops at the first child that
        does not exit 0; exit status 1 if any line differs

Cases: every ``SHAPES`` entry of tests/test_edit_knn_gpu.py, tests/test_edit_long_gpu.py (and its ``far_case``) and
tests/test_field_knn_gpu.py, every ``CASES`` entry of tests/test_field_weights_gpu.py, and the 65 x 257 x 48 rows of the field
suite under tables of F = 1, 4, 5 and 16 fields (every group count of the kernel), each without weights and with them.  Per case:
``*_distances`` (the matrix), ``*_knn_rows`` (head, rows, nbr) and ``*_knn_logp`` over 7 classes for both weightings and both
``normalize`` settings (the float32 log-probs).  The case builders form the restatements' outputs too; only the device's are
summed here."""
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

V = 7
FIELDS = (1, 4, 5, 16)
CHILD_SECONDS = 240


def crc(*tensors):
    return [zlib.crc32(t.detach().cpu().contiguous().numpy().tobytes()) for t in tensors]


def votes(torch, logp, buf, Lq, Lr, nr, **metric):
    """The four votes of a search's neighbours -> {name: crc}"""
    yr = (torch.arange(nr, device="cuda") * 5) % V
    prior = torch.softmax(torch.arange(V, dtype=torch.float64, device="cuda") / V, dim=0)
    return {f"logp_{w}_{int(n)}": crc(logp(buf, Lq, Lr, yr, prior, weights=w, normalize=n, tau=0.75, lam=0.5, **metric))
            for w in ("uniform", "distance") for n in (False, True)}


def lines():
    import numpy as np
    import torch
    import test_edit_knn_gpu as short
    import test_edit_long_gpu as long
    import test_field_knn_gpu as field
    import test_field_weights_gpu as weighted
    from slnlp import ops
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rows = lambda buf: crc(buf["head"], buf["rows"], buf["nbr"])

    def inputs(c):
        S = c["S"]
        ex = None if c["exclude"] is None else dev(c["exclude"])
        return dev(c["Xq"])[:, :S], dev(c["Lq"]), dev(c["Xr"])[:, :c.get("Sr", S)], dev(c["Lr"]), ex

    for i in range(len(short.SHAPES)):
        c = short.case(i)
        Xq, Lq, Xr, Lr, ex = inputs(c)
        buf = ops.edit_knn_rows(Xq, Lq, Xr, Lr, c["k"], radius=short.RADIUS, exclude=ex)
        yield {"search": "edit", "case": short.IDS[i], "distances": crc(ops.edit_distances(Xq, Lq, Xr, Lr)), "rows": rows(buf),
               **votes(torch, ops.edit_knn_logp, buf, Lq, Lr, c["nr"])}
    for i in list(range(len(long.SHAPES))) + ["far"]:
        c = long.far_case() if i == "far" else long.case(i)
        Xq, Lq, Xr, Lr, ex = inputs(c)
        buf = ops.edit_long_knn_rows(Xq, Lq, Xr, Lr, c["k"], max_len=c["max_len"], radius=long.RADIUS, exclude=ex)
        yield {"search": "edit_long", "case": "far" if i == "far" else long.IDS[i],
               "distances": crc(ops.edit_long_distances(Xq, Lq, Xr, Lr, max_len=c["max_len"])), "rows": rows(buf),
               **votes(torch, ops.edit_long_knn_logp, buf, Lq, Lr, c["nr"], max_len=c["max_len"])}

    def field_lines(name, c, codes, gap, k, radius, w, unit):
        Xq, Lq, Xr, Lr, ex = inputs(c)
        table = dev(codes)
        buf = ops.field_knn_rows(Xq, Lq, Xr, Lr, table, k, gap=gap, radius=radius, exclude=ex, field_weights=w)
        return {"search": "field" if w is None else "field_w", "case": name,
                "distances": crc(ops.field_distances(Xq, Lq, Xr, Lr, table, gap, field_weights=w)), "rows": rows(buf),
                **votes(torch, ops.field_knn_logp, buf, Lq, Lr, c["nr"], F=unit)}

    for i in range(len(field.SHAPES)):
        c = field.case(i)
        yield field_lines(field.IDS[i], c, c["codes"], c["gap"], c["k"], c["radius"], None, c["F"])
    for name in weighted.CASES:
        c = weighted.case(name)
        yield field_lines(name, c, c["codes"], c["gap"], c["k"], c["radius"], c["w"], c["W"])
    c = field.case(3)                            # 65 x 257 x 48: two reference tiles, queries past a wave
    for F in FIELDS:
        codes = np.random.RandomState(900 + F).randint(0, 4, size=(field.VT, F)).astype(np.int32)
        w = tuple((1 + (f == 0)) * (f % 2 == 0) for f in range(F))
        yield field_lines(f"65x257x48 F{F}", c, codes, F, 5, F, None, F)
        yield field_lines(f"65x257x48 F{F} w{sum(w)}", c, codes, sum(w), 5, sum(w), w, sum(w))
    torch.cuda.synchronize()


def compare(variant, dest):
    runs = {}
    for lib in ("", variant):                                # one fresh process per library: this one never opens the GPU
        env = dict(os.environ)
        env.pop("SLNLP_PROBE_LIB", None)
        if lib:
            env["SLNLP_PROBE_LIB"] = lib
        got = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=CHILD_SECONDS)
        if got.returncode != 0:
            sys.exit(f"knn_bits: the run of {lib or 'the product library'} failed ({got.returncode}):\n{got.stderr[-2000:]}")
        runs[lib or "product"] = [json.loads(l) for l in got.stdout.splitlines() if l.startswith("{")]
    a, b = runs["product"], runs[variant]
    differing = [(x, y) for x, y in zip(a, b) if x != y]
    res = {"command": f"python tools/knn_bits.py --compare {variant}", "lines": len(a), "equal": len(a) == len(b) and not differing,
           "differing": differing, **runs}
    if dest:
        with open(dest, "w") as f:
            json.dump(res, f, indent=0)
            f.write("\n")
    print(f"knn_bits: {len(a)} lines of the product library, {len(b)} of {variant}: " + ("all equal" if res["equal"] else f"{len(differing)} DIFFER"))
    for x, y in differing[:10]:
        print("  ", x["search"], x["case"], {k: (x[k], y.get(k)) for k in x if x[k] != y.get(k)})
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
