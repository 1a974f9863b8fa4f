"""What the fourteen neighbour-search entry points (slnlp_edit_* / slnlp_edit_long_* / slnlp_field_*) refuse, and in which words:
a transcript of return codes and messages, recorded on the CPU.

    python tools/record_knn_refusals.py [--out tests/golden/knn_refusals.json]      # record from the built library
    python tools/record_knn_refusals.py --check tests/golden/knn_refusals.json      # replay a transcript, exit 1 on a difference

The library loads without a GPU and a refused call launches nothing, so every pointer here is a MADE-UP, suitably aligned address
(only ``fweights``, which the library reads on the host, is a real array).  One or two arguments are bad per case; the cases with
two pin THE ORDER of the checks (null side before k, k before radius, radius before scratch, the table before the outputs).  Every
case must be refused with SLNLP_ERR_INVALID_ARG (-1 from a *_scratch_bytes): ``run`` stops at the first call that is not, so at most
one launch could ever see a made-up address.  tests/test_knn_refusals_cpu.py replays tests/golden/knn_refusals.json, which holds
every entry's good arguments once and per case the replaced ones beside the outcome, through ``replay``.  A refactor of the host
side records the transcript from the PARENT commit's library and holds the new one to it."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NQ, NR, LD, K, V = 3, 5, 8, 2, 4
BIG = 2 ** 30 + 1                                            # one row more than SLNLP_EDIT_MAX_ROWS
INVALID_ARG = 1                                              # SLNLP_ERR_INVALID_ARG


def addr(i):
    """The i-th made-up address: 16 MiB apart (no span of these cases is longer), 4 KiB aligned"""
    return 0x7F0000000000 + i * 0x1000000


SIDES = dict(Xq=addr(1), ldq=LD, Lq=addr(2), nq=NQ, Xr=addr(3), ldr=LD, Lr=addr(4), nr=NR)
TABLE = dict(codes=addr(5), Vt=20, F=6)
OUTS = dict(exclude=addr(6), k=K, radius=1, scratch=addr(7), scratch_bytes=2 * NQ * NR, head=addr(8), rows=addr(9), nbr=addr(10))
VOTE = dict(nbr=addr(10), rows=addr(9), Lq=addr(2), Lr=addr(4), yr=addr(11), nq=NQ, nr=NR, k=K, V=V)
VOTE_TAIL = dict(weights=1, tau=1.0, normalize=1, lam=1.0, prior=addr(12), logp=addr(13), ld=V, head=addr(8), stream=0)
WEIGHTS = [4, 0, 2, 0, 1, 3]                                 # W = 10

# entry -> its arguments in order with values the library accepts (width: the bytes of a matrix element; bound: the largest radius)
ENTRIES = {
    "slnlp_edit_distances": dict(**SIDES, dist=addr(7), stream=0),
    "slnlp_edit_long_distances": dict(**SIDES, max_len=300, dist=addr(7), stream=0),
    "slnlp_field_distances": dict(**SIDES, **TABLE, gap=6, dist=addr(7), stream=0),
    "slnlp_field_distances_w": dict(**SIDES, **TABLE, fweights=WEIGHTS, gap=10, dist=addr(7), stream=0),
    "slnlp_edit_knn_rows": dict(**SIDES, **OUTS, stream=0),
    "slnlp_edit_long_knn_rows": dict(**SIDES, max_len=300, **OUTS, stream=0),
    "slnlp_field_knn_rows": dict(**SIDES, **TABLE, gap=6, **OUTS, stream=0),
    "slnlp_field_knn_rows_w": dict(**SIDES, **TABLE, fweights=WEIGHTS, gap=10, **OUTS, stream=0),
    "slnlp_edit_knn_logp": dict(**VOTE, **VOTE_TAIL),
    "slnlp_edit_long_knn_logp": dict(**VOTE, max_len=300, **VOTE_TAIL),
    "slnlp_field_knn_logp": dict(**VOTE, F=6, **VOTE_TAIL),
    "slnlp_edit_knn_scratch_bytes": dict(nq=NQ, nr=NR),
    "slnlp_edit_long_knn_scratch_bytes": dict(nq=NQ, nr=NR),
    "slnlp_field_knn_scratch_bytes": dict(nq=NQ, nr=NR),
}
WIDTH = {"slnlp_edit_distances": 1, "slnlp_edit_knn_rows": 1}                     # every other matrix: 2 bytes
BOUND = {"slnlp_edit_knn_rows": 64, "slnlp_edit_long_knn_rows": 300, "slnlp_field_knn_rows": 64 * 6, "slnlp_field_knn_rows_w": 64 * 10}


def cases():
    """-> [(entry, case name, {argument: value})]: the one or two arguments that replace the entry's good ones"""
    out = []
    for entry, good in ENTRIES.items():
        def bad(name, **changes):
            assert set(changes) <= set(good), (entry, name)
            out.append((entry, name, changes))
        width = WIDTH.get(entry, 2)
        if entry.endswith("_scratch_bytes"):
            for key in ("nq", "nr"):
                bad(f"{key}=0", **{key: 0})
                bad(f"{key} above the rows", **{key: BIG})
            bad("too many pairs", nq=2 ** 16, nr=2 ** 16)
            continue
        if entry.endswith("_logp"):
            for key in ("nbr", "rows", "Lq", "Lr", "yr", "prior", "logp", "head"):
                bad(f"null {key}", **{key: None})
                bad(f"misaligned {key}", **{key: good[key] + (2 if key in ("nbr", "rows", "logp") else 4)})
            for key, low, high in (("nq", 0, BIG), ("nr", 0, BIG), ("k", 0, 65), ("V", 0, 2 ** 31), ("weights", -1, 2), ("normalize", -1, 2)):
                bad(f"{key}={low}", **{key: low})
                bad(f"{key}={high}", **{key: high})
            for key in ("tau", "lam"):
                for value in (0.0, -1.0, float("inf"), float("nan")):
                    bad(f"{key}={value}", **{key: value})
            bad("ld below V", ld=V - 1)
            bad("logp overlaps nbr", logp=good["nbr"])
            bad("head overlaps prior", head=good["prior"])
            bad("head overlaps logp", head=good["logp"])
            for key, high in (("max_len", 513), ("F", 17)):
                if key in good:
                    bad(f"{key}=0", **{key: 0})
                    bad(f"{key}={high}", **{key: high})
                    bad(f"{key}=0 and null nbr", **{key: 0, "nbr": None})
            bad("null nbr and k=0", nbr=None, k=0)
            bad("k=0 and V=0", k=0, V=0)
            continue
        rows = entry.endswith("_knn_rows") or entry.endswith("_knn_rows_w")
        for key in ("Xq", "Lq", "Xr", "Lr"):
            bad(f"null {key}", **{key: None})
            bad(f"misaligned {key}", **{key: good[key] + 4})
        for key in ("nq", "nr"):
            bad(f"{key}=0", **{key: 0})
            bad(f"{key} above the rows", **{key: BIG})
        for key in ("ldq", "ldr"):
            bad(f"{key}=0", **{key: 0})
            bad(f"{key} not addressable", **{key: 2 ** 62})
        bad("too many pairs", nq=2 ** 16, nr=2 ** 16)
        if "max_len" in good:
            bad("max_len=0", max_len=0)
            bad("max_len=513", max_len=513)
            bad("max_len=0 and null Xq", max_len=0, Xq=None)
        if "codes" in good:
            unit = sum(WEIGHTS) if "fweights" in good else good["F"]
            bad("null codes", codes=None)
            bad("misaligned codes", codes=good["codes"] + 2)
            for key, low, high in (("F", 0, 17), ("Vt", 0, 2 ** 31), ("gap", 0, unit + 1)):
                bad(f"{key}={low}", **{key: low})
                bad(f"{key}={high}", **{key: high})
            bad("null Lr and null codes", Lr=None, codes=None)
            bad("F=0 and too many pairs", F=0, nq=2 ** 16, nr=2 ** 16)
            bad("bad table and null output", Vt=0, **({"scratch": None, "nbr": None} if rows else {"dist": None}))
            if "fweights" in good:
                bad("null fweights", fweights=None)
                bad("null codes and null fweights", codes=None, fweights=None)
                bad("null fweights and F=0", fweights=None, F=0)
                bad("a weight of -1", fweights=[4, 0, -1, 0, 1, 3])
                bad("a weight of 17", fweights=[0, 0, 17, 0, 0, 0])
                bad("weights that sum to 0", fweights=[0] * 6)
                bad("weights that sum to 17", fweights=[4, 4, 4, 4, 1, 0])
                bad("a weight of 17 and gap=0", fweights=[0, 0, 17, 0, 0, 0], gap=0)
        if not rows:
            bad("null dist", dist=None)
            if width == 2:
                bad("misaligned dist", dist=good["dist"] + 1)
                bad("misaligned dist and too many pairs", dist=good["dist"] + 1, nq=2 ** 16, nr=2 ** 16)
            bad("null dist and too many pairs", dist=None, nq=2 ** 16, nr=2 ** 16)
            bad("dist overlaps Xq", dist=good["Xq"])
            bad("dist overlaps the end of Xq", dist=good["Xq"] + ((NQ - 1) * LD + LD) * 8 - 2)
            bad("dist overlaps Lr", dist=good["Lr"])
            if "codes" in good:
                bad("dist overlaps codes", dist=good["codes"])
            continue
        need, bound = width * NQ * NR, BOUND[entry]
        for key in ("scratch", "head", "rows", "nbr"):
            bad(f"null {key}", **{key: None})
        for key, off in (("head", 4), ("exclude", 4), ("rows", 2), ("nbr", 2)) + ((("scratch", 1),) if width == 2 else ()):
            bad(f"misaligned {key}", **{key: good[key] + off})
        for key, low, high in (("k", 0, 65), ("radius", -1, bound + 1)):
            bad(f"{key}={low}", **{key: low})
            bad(f"{key}={high}", **{key: high})
        bad("a short scratch", scratch_bytes=need - 1)
        bad("a negative scratch", scratch_bytes=-1)
        bad("scratch overlaps Xq", scratch=good["Xq"])
        bad("head overlaps Lq", head=good["Lq"])
        bad("rows overlaps exclude", rows=good["exclude"])
        bad("nbr overlaps Xr", nbr=good["Xr"])
        bad("nbr overlaps rows", nbr=good["rows"])
        bad("head overlaps scratch", head=good["scratch"] + 8)
        if "codes" in good:
            bad("scratch overlaps codes", scratch=good["codes"])
        bad("null side and bad k", Xr=None, k=0)
        bad("null output and too many pairs", head=None, nq=2 ** 16, nr=2 ** 16)
        bad("too many pairs and bad k", nq=2 ** 16, nr=2 ** 16, k=65)
        bad("bad k and bad radius", k=65, radius=bound + 1)
        bad("bad radius and short scratch", radius=-1, scratch_bytes=0)
        bad("short scratch and misaligned head", scratch_bytes=need - 1, head=good["head"] + 4)
        bad("misaligned rows and an overlap", rows=good["rows"] + 2, nbr=good["Xr"])
    return out


def run(lib, entries, cases):
    """Call every case -> [{entry, case, args, rc, message}], args the replaced arguments (a float as its repr).  Raises at the
    first call the library does not refuse with SLNLP_ERR_INVALID_ARG: nothing more is called then."""
    lib.slnlp_last_error.restype = C.c_char_p
    out = []
    for entry, name, changes in cases:
        args = {**entries[entry], **changes}
        host = {key: (C.c_int32 * len(v))(*v) for key, v in args.items() if isinstance(v, list)}       # alive across the call
        rc = getattr(lib, entry)(*(host.get(key, v) for key, v in args.items()))
        want = -1 if entry.endswith("_scratch_bytes") else INVALID_ARG
        message = lib.slnlp_last_error().decode(errors="replace")
        if rc != want:
            raise SystemExit(f"record_knn_refusals: {entry} ({name}) returned {rc}, not the refusal {want}: {message!r} -- stopping here")
        out.append({"entry": entry, "case": name, "args": {key: repr(v) if isinstance(v, float) else v for key, v in changes.items()},
                    "rc": rc, "message": message})
    return out


def replay(lib, recorded):
    """The cases of a transcript {"entries": the good arguments, "cases": [...]} called again, from the file alone -> what ``run``
    returns"""
    floats = lambda args: {key: float(v) if isinstance(v, str) else v for key, v in args.items()}
    return run(lib, {e: floats(good) for e, good in recorded["entries"].items()},
               [(c["entry"], c["case"], floats(c["args"])) for c in recorded["cases"]])


def load_library():
    sys.path.insert(0, os.path.join(ROOT, "sign-language-nlp_amd"))
    from slnlp import _lib
    return _lib.load()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--check", default=None, help="a transcript to replay against the built library")
    args = ap.parse_args()
    lib = load_library()
    if args.check:
        with open(args.check) as f:
            recorded = json.load(f)
        got = replay(lib, recorded)
        diff = [(a, b) for a, b in zip(recorded["cases"], got) if a != b]
        for a, b in diff[:20]:
            print(f"{a['entry']} ({a['case']}):\n  recorded {a['rc']} {a['message']!r}\n  now      {b['rc']} {b['message']!r}")
        print(f"{len(got)} cases, {len(diff)} differ")
        return 1 if diff else 0
    got = run(lib, ENTRIES, cases())
    good = {e: {key: repr(v) if isinstance(v, float) else v for key, v in args.items()} for e, args in ENTRIES.items()}
    text = '{"entries": ' + json.dumps(good) + ',\n"cases": [\n' + ",\n".join(json.dumps(c) for c in got) + "\n]}\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(f"{len(got)} refusals over {len(ENTRIES)} entry points" + (f" -> {args.out}" if args.out else ""), file=sys.stderr)
    if not args.out:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
