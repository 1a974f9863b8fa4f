#!/usr/bin/env python3
"""Record the layout of every packed judging buffer of ``slnlp.ops`` and what its download cuts out of it, on the CPU device.

    python tools/record_layouts.py [--out tests/golden/packed_layouts.json]

``record()`` builds every ``*_buffers`` result over CASES and returns ``{"layouts": ..., "downloads": ...}``:

* layouts: for every tensor reachable from a result (members of tuples included) its byte offset from the start of the allocation,
  byte length, dtype and shape, and the byte length of the allocation; for every scalar key (``shape``, ``end``, ``head``, the
  entries of ``at``) its value.
* downloads: the allocation's bytes are set to a pattern with no short period, ``(i * 2654435761) >> 7`` of the byte index i, so no
  two pieces look alike; then every ``*_download`` runs with each of its flags and every array it returns is recorded as dtype,
  shape and the CRC-32 of its bytes (anything else by its ``repr``).  ``reliability_download`` and ``ranking_download`` hand their
  table to ``metrics``: for those the table that arrives there is recorded.  The tuple downloads run a second time on clones of
  the tensors in separate allocations ("apart").

tests/golden/packed_layouts.json is written from the commit BEFORE a change to the packing and compared against the tree after it
(tests/test_packed_layouts_cpu.py), so the file is regenerated only when a layout is meant to move.  The grid holds the smallest
shapes at which a padding rule flips: N odd and even, N = 2049 (selective's second chunk word), V = 32 / 33 (one / two conformal
set words), 3 V + 1 odd and even, B (3 V + 1) odd, odd and even variant counts.
"""
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sign-language-nlp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

POINTS = ((1, 1), (2, 3), (5, 32), (8, 33), (2049, 202))     # (N, V)


def cases(ops, np):
    """-> [(name, make() -> the *_buffers result, [(label, download(result))])]"""
    out = []
    for N, V in POINTS:
        at = f"N{N}_V{V}"
        out.append((f"score_{at}", lambda N=N, V=V: ops.score_buffers(N, V, "cpu"), [("", ops.score_download)]))
        for bins in (1, 15):
            out.append((f"reliability_{at}_bins{bins}", lambda N=N, bins=bins: ops.reliability_buffers(N, bins, "cpu"),
                        [("", ops.reliability_download)]))
        for per_row in (True, False):
            out.append((f"ranking_{at}_rows{int(per_row)}", lambda N=N, V=V, per_row=per_row: ops.ranking_buffers(N, V, "cpu", per_row=per_row),
                        [("", ops.ranking_download)] + ([("per_row", lambda o: ops.ranking_download(o, per_row=True))] if per_row else [])))
        for k in (1, 3):
            out.append((f"topk_{at}_k{k}", lambda N=N, k=k: ops.topk_buffers(N, k, "cpu"), [("", ops.topk_download)]))
        for sets in (True, False):
            out.append((f"conformal_{at}_sets{int(sets)}", lambda N=N, V=V, sets=sets: ops.conformal_buffers(N, V, "cpu", sets=sets),
                        [("", ops.conformal_download), ("all", lambda b, sets=sets: ops.conformal_download(b, rows=True, sets=sets, score=True))]))
        out.append((f"selective_{at}", lambda N=N: ops.selective_buffers(N, "cpu"),
                    [("", ops.selective_download), ("lean", lambda b: ops.selective_download(b, counts=False))]))
        for k, M in ((None, 1), (1, 20), (3, 64)):
            k = k and min(k, V)
            out.append((f"error_analysis_{at}_k{k}_M{M}", lambda N=N, V=V, k=k, M=M: ops.error_analysis_buffers(N, V, k, M, "cpu"),
                        [(f"matrix{int(m)}_topk{int(t)}", lambda b, m=m, t=t: ops.error_analysis_download(b, matrix=m, topk=t))
                         for m in (True, False) for t in (True, False)]))
        for M in (1, 20, 64):
            out.append((f"label_audit_{at}_M{M}", lambda N=N, V=V, M=M: ops.label_audit_buffers(N, V, M, "cpu"),
                        [("", ops.label_audit_download), ("per_row", lambda b: ops.label_audit_download(b, per_row=True))]))
        for M, nb in ((3, 1), (4, 8)):
            variants = np.stack([np.arange(M) % N, np.arange(M), np.arange(M) % nb], axis=1).astype(np.int32)
            start = np.minimum(np.arange(N + 1), 1).astype(np.int32) * M
            out.append((f"attribution_{at}_M{M}_bins{nb}",
                        lambda N=N, V=V, variants=variants, start=start, nb=nb: ops.attribution_buffers(N, V, variants, start, nb, "cpu"),
                        [("", ops.attribution_download), ("per_variant", lambda b: ops.attribution_download(b, per_variant=True))]))
        for counts in (True, False):
            out.append((f"bootstrap_{at}_counts{int(counts)}", lambda V=V, counts=counts: ops.bootstrap_buffers(3, V, 3, counts, "cpu"),
                        [("", ops.bootstrap_download)]))
        for B, bins in ((1, 1), (7, 15)):
            out.append((f"score_interval_{at}_B{B}_bins{bins}", lambda N=N, V=V, B=B, bins=bins: ops.score_interval_buffers(N, V, B, "cpu", bins=bins),
                        [("", ops.score_interval_download)]))
    for Q in (0, 3):                                         # B (3 V + 1) odd: the int32 counts end inside a float64 word
        out.append((f"bootstrap_B7_V2_Q{Q}", lambda Q=Q: ops.bootstrap_buffers(7, 2, Q, True, "cpu"), [("", ops.bootstrap_download)]))
    return out


def tensors_of(torch, result, prefix=""):
    """-> [(path, tensor)] of every tensor reachable from a *_buffers result"""
    items = result.items() if isinstance(result, dict) else enumerate(result) if isinstance(result, (tuple, list)) else ()
    found = []
    for key, value in items:
        if torch.is_tensor(value):
            found.append((f"{prefix}{key}", value))
        elif isinstance(value, (dict, tuple, list)):
            found += tensors_of(torch, value, f"{prefix}{key}.")
    return found


def scalars_of(result, prefix=""):
    """-> {path: int} of every integer reachable through dicts, tuples and lists"""
    items = result.items() if isinstance(result, dict) else enumerate(result) if isinstance(result, (tuple, list)) else ()
    found = {}
    for key, value in items:
        if isinstance(value, int) and not isinstance(value, bool):
            found[f"{prefix}{key}"] = value
        elif isinstance(value, (dict, tuple, list)):
            found.update(scalars_of(value, f"{prefix}{key}."))
    return found


def layout(torch, result):
    got = {"scalars": scalars_of(result) if isinstance(result, dict) else {}, "tensors": {}}
    got["allocations"] = sorted({t.untyped_storage().data_ptr(): t.untyped_storage().nbytes() for _, t in tensors_of(torch, result)}.values())
    for path, t in tensors_of(torch, result):
        got["tensors"][path] = {"offset": t.data_ptr() - t.untyped_storage().data_ptr(), "bytes": t.numel() * t.element_size(),
                                "dtype": str(t.dtype), "shape": list(t.shape)}
    return got


def fill(torch, np, result):
    """set every byte of the allocation behind ``result`` to the pattern"""
    for storage in {t.untyped_storage().data_ptr(): t.untyped_storage() for _, t in tensors_of(torch, result)}.values():
        n = storage.nbytes()
        pattern = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)).astype(np.uint8)
        torch.empty(0, dtype=torch.uint8).set_(storage, 0, (n,)).copy_(torch.from_numpy(pattern))


def described(np, value):
    if isinstance(value, np.ndarray):
        return {"dtype": str(value.dtype), "shape": list(value.shape), "crc": zlib.crc32(np.ascontiguousarray(value).tobytes())}
    if isinstance(value, dict):
        return {str(k): described(np, v) for k, v in value.items()}
    if isinstance(value, (tuple, list)):
        return [described(np, v) for v in value]
    return repr(value.item() if isinstance(value, np.generic) else value)


def record():
    import numpy as np
    import torch
    from slnlp import metrics, ops
    table = []
    seen = lambda t: table.append(np.array(t)) or {}         # what metrics is handed, instead of the scores of a byte pattern
    real = metrics.reliability_from_table, metrics.ranking_from_table
    metrics.reliability_from_table = metrics.ranking_from_table = seen
    got = {"layouts": {}, "downloads": {}}
    try:
        for name, make, downloads in cases(ops, np):
            result = make()
            got["layouts"][name] = layout(torch, result)
            fill(torch, np, result)
            runs = list(downloads)
            if isinstance(result, tuple):
                apart = tuple(None if t is None else t.clone() for t in result)
                runs += [(f"{label}apart", lambda _, fn=fn: fn(apart)) for label, fn in downloads]
            for label, fn in runs:
                del table[:]
                value = fn(result)
                got["downloads"][f"{name}:{label}"] = described(np, {"result": value, "handed_to_metrics": list(table)})
    finally:
        metrics.reliability_from_table, metrics.ranking_from_table = real
    return got


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "tests", "golden", "packed_layouts.json")
    got = record()
    with open(out, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(got['layouts'])} layouts, {len(got['downloads'])} downloads -> {out}")
