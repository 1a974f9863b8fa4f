#!/usr/bin/env python3
"""Compare kernels of two device-assembly listings (hipcc ... --cuda-device-only -S file.hip -o file.s), host only.

    python tools/diff_kernel_isa.py parent.s new.s --kernels sgd_kernel adam_kernel ...
    python tools/diff_kernel_isa.py parent.s new.s            # every kernel both listings define

Per kernel (matched by substring of the mangled name; a name that matches several symbols must be one's exact demangled
base name, e.g. sgd_kernel does not match sgd_groups_kernel):
  (a) resources: next_free_vgpr / next_free_sgpr / group_segment_fixed_size / private_segment_fixed_size / scratch lines;
  (b) the instruction stream between the kernel's label and the function's end (every exit, not only the first s_endpgm),
      `.LBB<n>_<k>` labels renamed by the order in which the kernel defines them;
  (c) the multiset of opcodes.
Exit status 0: (a) equal for every kernel; 1 otherwise.  A differing stream with equal resources is reported, not an error.
"""
import argparse
import collections
import difflib
import re
import sys

RES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size",
       ".amdhsa_enable_private_segment", ".amdhsa_uses_dynamic_stack", ".amdhsa_accum_offset")


def parse(path):
    """-> {symbol: {"res": {...}, "stream": [instruction lines]}}"""
    out, cur, body = {}, None, None
    desc = None
    for raw in open(path, errors="replace"):
        line = raw.split(";")[0].rstrip()
        s = line.strip()
        if not s:
            continue
        m = re.match(r"^([A-Za-z_][\w$.]*):$", s)
        if m and not s.startswith(".L") and body is None and not line[0].isspace():
            cur, body = m.group(1), []
            continue
        if body is not None:
            if re.match(r"^\.LBB\d+_\d+:$", s):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
            elif s.startswith((".section", ".Lfunc_end")):   # the function's end (its descriptor's section follows the last
                                                             # instruction): an early-exit s_endpgm does not end the stream
                out.setdefault(cur, {})["stream"] = body
                body = None
            elif s.startswith("."):
                pass                                # directives inside a body (.p2align ...)
            else:
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", s)))
            continue
        m = re.match(r"^\.amdhsa_kernel\s+(\S+)", s)
        if m:
            desc = m.group(1)
            out.setdefault(desc, {})["res"] = {}
            continue
        if s.startswith(".end_amdhsa_kernel"):
            desc = None
        elif desc and s.split()[0] in RES:
            out[desc]["res"][s.split()[0]] = s.split()[1]
    for v in out.values():                          # a block's number shifts with every block in front of it: name the labels
        if "stream" in v:                           # of a kernel by the order in which it defines them
            names = {}
            for l in v["stream"]:
                if l.startswith(".LBB_") and l.endswith(":"):
                    names[l[:-1]] = f".L{len(names)}"
            v["stream"] = [re.sub(r"\.LBB_\d+", lambda m: names.get(m.group(0), m.group(0)), l) for l in v["stream"]]
    return {k: v for k, v in out.items() if "stream" in v and "res" in v}


def pick(table, name):
    hits = [k for k in table if name in k]
    exact = [k for k in hits if f"{len(name)}{name}" in k]        # the Itanium mangling of the base name
    hits = exact or hits
    if len(hits) != 1:
        sys.exit(f"{name}: {len(hits)} symbols match ({', '.join(hits[:4])})")
    return hits[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--kernels", nargs="*", help="kernel names (default: every symbol both listings define)")
    ap.add_argument("--show", type=int, default=12, help="differing stream lines to print per kernel")
    a = ap.parse_args()
    A, B = parse(a.parent), parse(a.new)
    if a.kernels:
        pairs = [(n, pick(A, n), pick(B, n)) for n in a.kernels]
    else:
        both = sorted(set(A) & set(B))
        pairs = [(k, k, k) for k in both]
        for k in sorted(set(A) ^ set(B)):
            print(f"only in {'parent' if k in A else 'new'}: {k}")
    bad = 0
    for name, ka, kb in pairs:
        ra, rb = A[ka]["res"], B[kb]["res"]
        sa, sb = A[ka]["stream"], B[kb]["stream"]
        res = " ".join(f"{k.replace('.amdhsa_', '')}={v}" for k, v in sorted(rb.items()) if k in RES[:4])
        ca, cb = collections.Counter(l.split()[0] for l in sa), collections.Counter(l.split()[0] for l in sb)
        verdict = "stream identical" if sa == sb else "stream DIFFERS"
        print(f"{name}: resources {'equal' if ra == rb else 'DIFFER'} ({res}); {len(sa)} -> {len(sb)} lines, {verdict}; "
              f"opcode multiset {'equal' if ca == cb else 'DIFFERS'}")
        if ra != rb:
            bad = 1
            for k in sorted(set(ra) | set(rb)):
                if ra.get(k) != rb.get(k):
                    print(f"    {k}: {ra.get(k)} -> {rb.get(k)}")
        if ca != cb:
            for op in sorted(set(ca) | set(cb)):
                if ca[op] != cb[op]:
                    print(f"    {op}: {ca[op]} -> {cb[op]}")
        if sa != sb:
            shown = 0
            for l in difflib.unified_diff(sa, sb, "parent", "new", lineterm="", n=0):
                if shown >= a.show:
                    print("    ...")
                    break
                print("    " + l)
                shown += 1
    return bad


if __name__ == "__main__":
    sys.exit(main())
