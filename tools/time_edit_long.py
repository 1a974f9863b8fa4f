"""Cost of the edit-distance neighbour search of rows longer than 64 frames (``slnlp_edit_long_distances`` / ``_knn_rows`` /
``_knn_logp``, csrc/edit_long.hip: ``slnlp.EditKNN(max_len=...)``, ``slnlp.split_audit(..., max_len=...)``), and whether the
64-frame search beside it is what it was.

    python tools/time_edit_long.py [--out profiles/edit_long_timing.json] [--host-queries 8]
    python tools/time_edit_long.py --registers [--out profiles/edit_long_timing.json]        (no GPU: hipcc alone)
    python tools/time_edit_long.py --ab parent [--out profiles/knn_shell_timing.json]

Rows from ``synthetic_dataset`` (3000 source tokens, 200 labels, lengths 8..S), k = 5.  Event-timed as tools/time_edit_knn.py: one
``ops`` call between two HIP events, the second one waited for, into buffers allocated once; 5 warm-up calls, 30 samples;
``*_batched``: 10 calls between one pair of events, divided by 10.  No pass / fail: the numbers are recorded.

* ``short_path``: the UNTOUCHED ``ops.edit_knn_rows`` at 4000 x 4000, S = 48, each run in a fresh child process, in the order
  parent, this commit, parent.  The parent commit's library is ``lib/libslnlp_probeparent.so`` (build the parent commit's tree with
  ``make`` and copy its ``lib/libslnlp.so`` there; the child loads it through ``SLNLP_PROBE_LIB=parent``); where it is absent the
  parent's runs are recorded as not measured.  ``inside_parent_spread``: whether this commit's batched median lies between the
  parent's two; otherwise ``difference_us`` against the nearer one says by how much it does not.
* ``general_kernel_on_short_rows``: the long path (max_len 512) on the SAME S = 48 rows, where every query is one word: what the
  general kernel costs where the single-word one applies.
* ``long_rows``: the long path at S = max_len = 128, 256 and 512 for 800 x 3200 and 4000 x 4000: distances, rows, votes, the whole
  ``predict_proba`` (wall clock between two device synchronisations; 3 warm-up, 10 samples) and pairs per microsecond.
* ``scaling``: the work of a pair is ceil(m / 64) n word steps (m the query's length, n the reference's); per shape the sum of
  that count over all pairs, the distance kernel's batched median and their quotient, next to the same quotient of the single-word
  kernel on the S = 48 rows.
* ``host``: the numpy restatement (tests/edit_long_ref.py) on the FIRST ``--host-queries`` queries of one long shape, wall clock, and
  ``same_integers``: whether the device's neighbours of those queries equal it.  Not scaled to a claim about the full size.
* ``registers`` (``--registers``, merged into ``--out``): the register allocation, scratch and LDS bytes of ``edit_long_dist_kernel``
  from the code object's metadata -- of the built library, and of csrc/edit_long.hip compiled with one W alone
  (``-DSLNLP_EDIT_LONG_ONLY_W=W``) for each W the kernel instantiates.
* ``--ab NAME`` (a run of its own, whose parent process never opens the GPU; with ``--out`` it is merged into that file under
  ``edit_long_knn_rows_vs_parent``): ``ops.edit_long_knn_rows`` at 4000 x 4000, S = max_len = 128 -- a ``long_rows`` shape above --
  under the product library and under lib/libslnlp_probeNAME.so, in fresh child processes, interleaved, ``--ab-rounds`` times
  (tools/knn_ab.py): each child's batched median, per build the spread between its repeated medians; the margin is the parent's."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "sign-language-nlp_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

K, SRC_VOCAB, LABELS = 5, 3000, 200
SHORT_S, SHORT_N = 48, 4000
LONG_S = (128, 256, 512)
SHAPES = (("test_vs_train_800x3200", 800, 3200), ("leave_one_out_4000x4000", 4000, 4000))
WARMUP, SAMPLES, BATCH = 5, 30, 10
WORDS = (1, 2, 3, 4, 6, 8)                                   # the W csrc/edit_long.hip instantiates


def stats(v, unit):
    v = np.asarray(v)
    return {f"median_{unit}": float(np.median(v)), f"min_{unit}": float(v.min()), f"max_{unit}": float(v.max())}


def timed_us(fn, calls=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def sampled(fn):
    lone = stats([timed_us(fn) for _ in range(WARMUP + SAMPLES)][WARMUP:], "us")
    batched = stats([timed_us(fn, BATCH) for _ in range(3 + 10)][3:], "us")
    return lone, batched


def rows_of(S, n):
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(n, seq_len=S, src_vocab=SRC_VOCAB, n_labels=LABELS, seed=1, min_len=8)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def word_steps(Lq, Lr):
    """The sum over all pairs of ceil(m / 64) n"""
    return int(((np.asarray(Lq) + 63) // 64).sum()) * int(np.asarray(Lr).sum())


# ---------------------------------------------------------------------------------------------------- the short path ----
def short_path_child():
    """One process: the untouched edit_knn_rows (and edit_distances) at 4000 x 4000, S = 48, of whichever library is loaded"""
    import torch
    from slnlp import _lib, ops
    data = rows_of(SHORT_S, 2 * SHORT_N)
    train, test = data[np.arange(SHORT_N)], data[np.arange(SHORT_N, 2 * SHORT_N)]
    Xq, Lq, Xr, Lr = dev(test.ids), dev(test.lengths), dev(train.ids), dev(train.lengths)
    scratch = torch.empty(SHORT_N * SHORT_N, dtype=torch.uint8, device="cuda")
    dist = torch.empty(SHORT_N, SHORT_N, dtype=torch.uint8, device="cuda")
    buf = ops.edit_knn_buffers(SHORT_N, K, "cuda")
    res = {"library": os.path.basename(_lib.LIB_PATH)}
    res["knn_rows"], res["knn_rows_batched"] = sampled(lambda: ops.edit_knn_rows(Xq, Lq, Xr, Lr, K, buf=buf, scratch=scratch))
    res["distances"], res["distances_batched"] = sampled(lambda: ops.edit_distances(Xq, Lq, Xr, Lr, out=dist))
    res["word_steps"] = word_steps(test.lengths, train.lengths)
    print("SHORT_PATH " + json.dumps(res))


def short_path():
    parent = os.path.join(PKG, "lib", "libslnlp_probeparent.so")
    runs = []
    for which in ("parent", "this", "parent"):
        if which == "parent" and not os.path.exists(parent):
            runs.append({"commit": which, "not_measured": "lib/libslnlp_probeparent.so is absent"})
            continue
        env = dict(os.environ)
        env.pop("SLNLP_PROBE_LIB", None)
        if which == "parent":
            env["SLNLP_PROBE_LIB"] = "parent"
        print(f"[time_edit_long] short path, {which} commit ...", file=sys.stderr, flush=True)
        done = subprocess.run([sys.executable, HERE, "--short-path-child"], env=env, stdout=subprocess.PIPE, text=True, timeout=300)
        line = [l for l in done.stdout.splitlines() if l.startswith("SHORT_PATH ")]
        runs.append({"commit": which, **json.loads(line[-1][len("SHORT_PATH "):])} if done.returncode == 0 and line
                    else {"commit": which, "not_measured": f"the child ended with status {done.returncode}"})
    res = {"shape": f"{SHORT_N} x {SHORT_N}, S = {SHORT_S}, k = {K}", "order": "parent, this commit, parent: a fresh process each", "runs": runs}
    med = [r["knn_rows_batched"]["median_us"] if "knn_rows_batched" in r else None for r in runs]
    if None not in med:
        lo, hi = min(med[0], med[2]), max(med[0], med[2])
        res["parent_knn_rows_batched_median_us"], res["this_knn_rows_batched_median_us"] = [med[0], med[2]], med[1]
        res["inside_parent_spread"] = bool(lo <= med[1] <= hi)
        if not res["inside_parent_spread"]:
            near = lo if med[1] < lo else hi
            res["difference_us"], res["difference_relative"] = med[1] - near, (med[1] - near) / near
    return res


# ----------------------------------------------------------------------------------------------------- the long path ----
def time_long(name, nq, nr, S, max_len, data, host_queries=0):
    import torch
    import edit_long_ref as R
    import slnlp
    from slnlp import ops
    print(f"[time_edit_long] {name}, S = {S}, max_len = {max_len} ...", file=sys.stderr, flush=True)
    train, test = data[np.arange(nr)], data[np.arange(nr, nr + nq)]
    V = len(data.vocab_y)
    Xq, Lq, Xr, Lr, yr = dev(test.ids), dev(test.lengths), dev(train.ids), dev(train.lengths), dev(train.y)
    prior = dev(R.prior_of(train.y, V))
    dist = torch.empty(nq, nr, dtype=torch.uint16, device="cuda")
    scratch = torch.empty(2 * nq * nr, dtype=torch.uint8, device="cuda")
    buf = ops.edit_knn_buffers(nq, K, "cuda")
    logp = torch.empty(nq, V, dtype=torch.float32, device="cuda")
    res = {"name": name, "nq": nq, "nr": nr, "S": S, "max_len": max_len, "k": K, "V": V, "pairs": nq * nr, "scratch_bytes": 2 * nq * nr,
           "mean_query_words": float(((test.lengths + 63) // 64).mean()), "mean_reference_length": float(train.lengths.mean())}
    for key, fn in (("distances", lambda: ops.edit_long_distances(Xq, Lq, Xr, Lr, max_len=max_len, out=dist)),
                    ("knn_rows", lambda: ops.edit_long_knn_rows(Xq, Lq, Xr, Lr, K, max_len=max_len, buf=buf, scratch=scratch)),
                    ("knn_logp", lambda: ops.edit_long_knn_logp(buf, Lq, Lr, yr, prior, max_len=max_len, out=logp))):
        res[key], res[key + "_batched"] = sampled(fn)
    res["pairs_per_us"] = nq * nr / res["distances_batched"]["median_us"]
    res["word_steps"] = word_steps(test.lengths, train.lengths)
    res["word_steps_per_ns"] = res["word_steps"] / (res["distances_batched"]["median_us"] * 1e3)
    if max_len > 64:
        knn = slnlp.EditKNN(k=K, max_len=max_len).fit(train)
        res["predict_proba"] = stats([wall_ms(lambda: knn.predict_proba(test))[0] for _ in range(3 + 10)][3:], "ms")
    if host_queries:
        m = min(host_queries, nq)
        t0 = time.perf_counter()
        d = R.distances(test.ids[:m], test.lengths[:m], train.ids, train.lengths, max_len)
        want = R.knn_rows(d, test.lengths[:m], train.lengths, S, S, K, max_len)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = ops.edit_knn_download(buf)
        res["host"] = {"queries_timed": m, "ms": host_ms, "note": f"the restatement on the first {m} of {nq} queries; not scaled to the full size"}
        res["same_integers"] = bool(np.array_equal(got["nbr"][:m], want["nbr"]) and np.array_equal(got["rows"][:m], want["rows"]))
    return res


def ab_child():
    """One child of the A / B: edit_long_knn_rows at 4000 x 4000, S = max_len = 128, batched medians of its own repeats"""
    import torch
    from slnlp import ops
    S, n = LONG_S[0], SHORT_N
    data = rows_of(S, 2 * n)
    Xr, Lr, Xq, Lq = dev(data.ids[:n]), dev(data.lengths[:n]), dev(data.ids[n:]), dev(data.lengths[n:])
    buf = ops.edit_knn_buffers(n, K, "cuda")
    scratch = torch.empty(2 * n * n, dtype=torch.uint8, device="cuda")
    fn = lambda: ops.edit_long_knn_rows(Xq, Lq, Xr, Lr, K, max_len=S, buf=buf, scratch=scratch)
    batched = stats([timed_us(fn, 4) for _ in range(2 + 9)][2:], "us")
    got = ops.edit_knn_download(buf)
    print(json.dumps({"knn_rows_batched": batched, "checksum": int(got["nbr"].astype(np.int64).sum())}))


# --------------------------------------------------------------------------------------------------------- registers ----
def kernel_metadata(path, match="edit_long"):
    import msgpack
    import struct
    import kernel_registers as kr
    out = {}
    for _, elf in kr.code_objects(open(path, "rb").read()):
        shoff, = struct.unpack_from("<Q", elf, 40)
        shentsize, shnum = struct.unpack_from("<HH", elf, 58)
        for i in range(shnum):
            sh = shoff + i * shentsize
            if struct.unpack_from("<I", elf, sh + 4)[0] != 7:
                continue
            off, size = struct.unpack_from("<QQ", elf, sh + 24)
            p = off
            while p + 12 <= off + size:
                namesz, descsz, ntype = struct.unpack_from("<III", elf, p)
                d0 = p + 12 + (namesz + 3) // 4 * 4
                if elf[p + 12:p + 12 + namesz].rstrip(b"\0") == b"AMDGPU" and ntype == 32:
                    for k in msgpack.unpackb(elf[d0:d0 + descsz], raw=False, strict_map_key=False).get("amdhsa.kernels", []):
                        if match in k.get(".name", ""):
                            short = k[".name"].split("slnlp")[1].lstrip("0123456789").split("ENS_")[0] if "slnlp" in k[".name"] else k[".name"]
                            out[short] = {"vgpr_count": k.get(".vgpr_count"), "agpr_count": k.get(".agpr_count", 0), "sgpr_count": k.get(".sgpr_count"),
                                          "scratch_bytes": k.get(".private_segment_fixed_size"), "lds_bytes": k.get(".group_segment_fixed_size"),
                                          "vgpr_spills": k.get(".vgpr_spill_count", 0)}
                p = d0 + (descsz + 3) // 4 * 4
    return out


def registers():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    res = {"instantiated_W": list(WORDS), "dispatch": "once per query inside the kernel, to the smallest instantiated W >= ceil(m / 64)",
           "library": kernel_metadata(os.path.join(PKG, "lib", "libslnlp.so")), "one_W_alone": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for W in WORDS:
            obj = os.path.join(tmp, f"edit_long_w{W}.o")
            subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-Xclang", "-target-feature",
                            "-Xclang", "-packed-fp32-ops", "-DSLNLP_PROBE_FENCES=0", f"-DSLNLP_EDIT_LONG_ONLY_W={W}", "-c",
                            os.path.join(PKG, "csrc", "edit_long.hip"), "-o", obj], check=True, stderr=subprocess.DEVNULL)
            res["one_W_alone"][str(W)] = kernel_metadata(obj, "edit_long_dist").get("edit_long_dist_kernel")
    res["note"] = ("library: the kernels as built, every W behind one branch; one_W_alone: csrc/edit_long.hip compiled with "
                   "-DSLNLP_EDIT_LONG_ONLY_W=W, the register count of that loop by itself.  gfx950: .vgpr_count is the wave's whole allocation")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-queries", type=int, default=8)
    ap.add_argument("--registers", action="store_true", help="only the register record (no GPU), merged into --out")
    ap.add_argument("--short-path-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--ab", default=None, help="NAME of lib/libslnlp_probeNAME.so, the parent commit's library")
    ap.add_argument("--ab-rounds", type=int, default=4)
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.short_path_child:
        return short_path_child()
    if args.ab_child:
        return ab_child()
    if args.ab:                                              # children only: this process stays off the GPU
        from knn_ab import ab
        res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        what = (f"ops.edit_long_knn_rows (distances, selection, head) at {SHORT_N} x {SHORT_N}, S = max_len = {LONG_S[0]}, k = {K}; 4 calls between one "
                "pair of events, median of 9 repeats per child process; children interleaved on one box")
        res["edit_long_knn_rows_vs_parent"] = ab(HERE, ["--ab-child"], args.ab, args.ab_rounds, what, "time_edit_long")
    elif args.registers:
        res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        res["registers"] = registers()
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/time_edit_long.py: no GPU -- nothing is measured without one")
        res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        keep = {"registers": res["registers"]} if "registers" in res else {}
        res = {"command": "python tools/time_edit_long.py --out profiles/edit_long_timing.json", "short_path": short_path()}     # children first: this
        res["device"] = torch.cuda.get_device_name(0)                                                                           # process has no GPU open yet
        short = rows_of(SHORT_S, 2 * SHORT_N)
        res["general_kernel_on_short_rows"] = time_long("leave_one_out_4000x4000", SHORT_N, SHORT_N, SHORT_S, 512, short)
        res["long_rows"] = []
        for S in LONG_S:
            data = rows_of(S, max(nq + nr for _, nq, nr in SHAPES))
            for name, nq, nr in SHAPES:
                res["long_rows"].append(time_long(name, nq, nr, S, S, data, args.host_queries if (S, nq) == (256, 800) else 0))
        this = [r for r in res["short_path"]["runs"] if r["commit"] == "this" and "distances_batched" in r]
        one = this[0]["word_steps"] / (this[0]["distances_batched"]["median_us"] * 1e3) if this else None
        res["scaling"] = {"unit": "word steps (the sum over all pairs of ceil(m / 64) n) per nanosecond of the distance kernel's batched median",
                          "single_word_kernel_S48_4000x4000": one,
                          "general_kernel_S48_4000x4000": res["general_kernel_on_short_rows"]["word_steps_per_ns"],
                          "long_rows": {f"{r['name']}_S{r['S']}": r["word_steps_per_ns"] for r in res["long_rows"]}}
        res["note"] = ("distances / knn_rows / knn_logp: HIP events around one ops call (1 / 3 / 2 launches), the second event waited for, "
                       f"{SAMPLES} samples after {WARMUP} warm-up; *_batched: {BATCH} calls between one pair of events, per call; predict_proba: wall "
                       "clock between two device synchronisations; host: the numpy restatement on a stated subset of the queries, not scaled")
        res.update(keep)
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
