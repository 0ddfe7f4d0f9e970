#!/usr/bin/env python3
"""What one trip of hamming_topk_fp4rows' main loop costs on the path every block but one in two thousand takes, read off the gfx950
assembly (no GPU: hipcc cross-compiles; same compiler, same flags as tod_amd/csrc/Makefile).

The loop is bound by vector issue ("What bounds the split-block kernel": cycles/block ~ 20 NM + 4 V), so every vector
instruction on that path is paid in full, copies at the back edge included -- and a count that stops in front of the back branch misses
those. This tool compiles match.hip with -S and, for each named instantiation <K, QT, MODE>, finds the kernel's main loop (the loop
whose fall-through path holds the most MFMAs) and walks that path from the loop's header to the branch back to it: a conditional branch
that leaves the path (a block that goes on, the exit) is not taken, an unconditional one is followed (--take names labels that a
conditional branch is followed to, for a build whose common path takes one). It reports the MFMAs, the other
v_ instructions, the v_mov_b32 among them, the buffer loads, s_nop and s_waitcnt on the path, and the kernel's registers and scratch.

    python tools/k4x_trip_counts.py 2,6,2 5,6,2 2,4,2            # one JSON line per instantiation
    python tools/k4x_trip_counts.py --asm match.s --path 2,6,2   # from an assembly file; the path's instructions to stderr

tests/test_match_trip_build.py holds the paired forms (MODE 2) to their counts."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only"]


def compile_asm(source=None):
    """match.hip (or `source`) as gfx950 assembly text"""
    source = source or os.path.join(ROOT, "tod_amd", "csrc", "match.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "out.s")
        subprocess.run([HIPCC] + FLAGS + ["-o", out, source], check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def kernel_pattern(k, qt, mode):
    return "hamming_topk_fp4rowsILi%dELi%dELi%dEE" % (k, qt, mode)


def kernel_body(asm, pattern):
    """(symbol, [instruction or label lines]) of the one kernel whose mangled name contains `pattern`"""
    found = [m for m in re.finditer(r"^(_Z\S*):", asm, re.M) if pattern in m.group(1) and not m.group(1).endswith(".kd")]
    if len(found) != 1:
        raise LookupError("%d kernels match %s" % (len(found), pattern))
    start = found[0].end()
    end = asm.find(".Lfunc_end", start)
    end = len(asm) if end < 0 else end
    lines = []
    for line in asm[start:end].split("\n"):
        ins = line.split(";")[0].strip()
        if ins and not ins.startswith(".") or re.match(r"\.LBB\d+_\d+:", ins):
            lines.append(ins)
    return found[0].group(1), lines


def kernel_resources(asm, symbol):
    """From the kernel's metadata map, whose keys are sorted: these three stand behind .name, in front of the next kernel's map"""
    m = re.search(r"\.name:\s+" + re.escape(symbol) + r"\s", asm)
    blk = asm[m.start():m.start() + 1500].split("\n  - ")[0]
    num = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
    return {"vgprs": num("vgpr_count"), "sgprs": num("sgpr_count"), "scratch_bytes": num("private_segment_fixed_size")}


def walk(lines, labels, header, take=()):
    """The fall-through path from label `header` to the branch back to it, or None if the path does not return there. take: labels
    a conditional branch IS followed to (a build whose common path runs through a taken branch)"""
    path, i, seen = [], labels[header] + 1, set()
    while i < len(lines) and i not in seen:
        seen.add(i)
        ins = lines[i]
        i += 1
        if ins.endswith(":"):
            continue
        op = ins.split()[0]
        if op == "s_endpgm" or op.startswith("s_setpc"):
            return None
        if op.startswith("s_cbranch") or op == "s_branch":
            target = ins.split()[-1]
            path.append(ins)
            if target == header:
                return path
            if op == "s_branch" or target in take:
                if target not in labels:
                    return None
                i = labels[target] + 1
            continue
        path.append(ins)
    return None


def trip_counts(asm, k, qt, mode, want_path=False, take=()):
    symbol, lines = kernel_body(asm, kernel_pattern(k, qt, mode))
    labels = {ins[:-1]: i for i, ins in enumerate(lines) if ins.endswith(":")}
    # a loop's header stands in front of the branch that returns to it; a label reached only from above is a join or a cold block
    headers = {ins.split()[-1] for i, ins in enumerate(lines)
               if (ins.startswith("s_cbranch") or ins.startswith("s_branch ")) and labels.get(ins.split()[-1], len(lines)) < i}
    best = None
    for header in sorted(headers):
        path = walk(lines, labels, header, take)
        if path is None:
            continue
        n = sum(p.startswith("v_mfma") for p in path)
        # (the masked whole-block steps behind the main loop can hold as many MFMAs: the main loop stands first)
        if best is None or n > best[0] or (n == best[0] and labels[header] < labels[best[1]]):
            best = (n, header, path)
    if best is None or best[0] == 0:
        raise LookupError("no loop with MFMAs in %s" % symbol)
    n_mfma, header, path = best
    ops = [p.split()[0] for p in path]
    valu = [o for o in ops if o.startswith("v_") and not o.startswith("v_mfma")]
    out = {"kernel": "hamming_topk_fp4rows<%d, %d, %d>" % (k, qt, mode), "loop_header": header, "instructions": len(path),
           "mfma": n_mfma, "valu": len(valu), "v_mov_b32": sum(o.startswith("v_mov_b32") for o in valu),
           "buffer_loads": sum(o.startswith("buffer_load") for o in ops), "s_nop": ops.count("s_nop"),
           "s_waitcnt": ops.count("s_waitcnt"), "branches": sum(o.startswith("s_cbranch") or o == "s_branch" for o in ops)}
    if mode == 2:
        out["pairs"] = n_mfma // 4
        out["valu_per_pair"] = round(len(valu) / (n_mfma // 4), 3)
    out.update(kernel_resources(asm, symbol))
    if want_path:
        out["path"] = path
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("forms", nargs="+", help="K,QT,MODE of an instantiation of hamming_topk_fp4rows, e.g. 2,6,2")
    ap.add_argument("--asm", help="read this assembly file instead of compiling tod_amd/csrc/match.hip")
    ap.add_argument("--source", help="compile this file instead of tod_amd/csrc/match.hip")
    ap.add_argument("--take", default="", help="comma-separated labels that a conditional branch is followed to")
    ap.add_argument("--path", action="store_true", help="print the instructions of each path to stderr")
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            asm = f.read()
    else:
        asm = compile_asm(a.source)
    for form in a.forms:
        k, qt, mode = (int(x) for x in form.split(","))
        r = trip_counts(asm, k, qt, mode, want_path=a.path, take=tuple(t for t in a.take.split(",") if t))
        for ins in r.pop("path", []):
            print("    " + ins, file=sys.stderr)
        print(json.dumps(r))


if __name__ == "__main__":
    main()
