"""Summary of a rocprofv3 --kernel-trace of the default bench.py command for profiles/verify_regs.json (tools/verify_regs.sh trace):
per verifier kernel the launches per batch, the grid in workgroups, the workgroup size, the duration beside the matcher, and the
registers, LDS and scratch the dispatch was made with; then, for the kernels whose allocation does not fit beside two waves of the
DB pass, waves x duration as a share of the device's 1024 SIMDs x the step time. That share is an ESTIMATE and an upper one: it
takes every wave of a launch to live as long as the launch.

Registers, LDS and scratch come from the code object: give the gfx950 assembly of verify.hip and match.hip (hipcc -S --cuda-device-only,
the Makefile's flags; tools/verify_regs.sh asm) behind the trace. rocprofv3's own VGPR_Count column is not the code object's figure
(it showed 100 for the pass's 196 and 80 for eval_kernel's 159, but 88 for growth_kernel's 84) and is printed only when no assembly is given.

usage: verify_regs_trace.py <kernel_trace.csv or .csv.gz> [verify.s match.s ...]"""
import csv
import gzip
import re
import statistics
import subprocess
import sys

SIMDS, FILE_REGS = 1024, 512
VERIFIER = re.compile(r"^(adjacency|finite|round_prep|invalidate|small_prep|cluster_frame|cluster_frame_rescaled|growth|eval|draw_table|draw_table_lane|"
                      r"chain|sprint|copy_words|depth_lookup|pnp_\w+)_kernel")   # the kernels of verify*.h and pnp.hip
PASS = re.compile(r"hamming_topk_fp4rows")


def short(name):
    return name.replace("(anonymous namespace)::", "").replace("tod::", "").replace("void ", "").split("(")[0]


def num(row, *keys):
    for k in keys:
        if row.get(k) not in (None, ""):
            return int(float(row[k]))
    return 0


def code_objects(paths):
    """{short demangled name: (vgpr, agpr, static LDS, scratch)} of every kernel in the assembly files"""
    out = {}
    for p in paths:
        asm = open(p).read()
        for e in re.split(r"\n  - ", asm[asm.index("amdhsa.kernels:"):])[1:]:
            m = re.search(r"\n    \.name:\s+(\S+)", e)      # (the kernel's own name, not an argument's)
            if not m or ".vgpr_count:" not in e:
                continue
            f = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, e).group(1))
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            out[short(name)] = (f("vgpr_count"), f("agpr_count"), f("group_segment_fixed_size"), f("private_segment_fixed_size"))
    return out


def main(path, asm_paths):
    co = code_objects(asm_paths)
    rows = list(csv.DictReader(gzip.open(path, "rt") if path.endswith(".gz") else open(path)))
    by = {}
    for r in rows:
        by.setdefault(short(r["Kernel_Name"]), []).append(r)
    passes = [n for n in by if PASS.search(n)]
    if not passes:
        sys.exit("no DB pass in the trace")
    main_pass = max(passes, key=lambda n: len(by[n]))
    p = by[main_pass]
    starts = sorted(int(r["Start_Timestamp"]) for r in p)
    step_us = statistics.median(b - a for a, b in zip(starts, starts[1:])) / 1e3
    regs = lambda n, r: co[n][:2] if n in co else (num(r, "VGPR_Count"), num(r, "Accum_VGPR_Count"))
    alloc = lambda n, r: -(-sum(regs(n, r)) // 8) * 8
    pass_alloc = alloc(main_pass, p[0])
    room = FILE_REGS - 2 * pass_alloc
    dur = lambda rs: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rs]
    print("DB pass %s: %d launches, %.1f us median, step %.1f us (median start to start), vgpr %d agpr %d -> allocation %d, room beside two waves %d"
          % (main_pass, len(p), statistics.median(dur(p)), step_us, regs(main_pass, p[0])[0], regs(main_pass, p[0])[1], pass_alloc, room))
    print("registers from %s" % ("the code objects" if co else "the trace's own columns"))
    batches = len(p)   # one verifier batch per step of the pipeline
    total_share = 0.0
    for n in sorted(by, key=lambda n: -sum(dur(by[n]))):
        if not VERIFIER.search(n):
            continue
        rs = by[n]
        d = dur(rs)
        wg = [num(r, "Workgroup_Size", "Workgroup_Size_X") * max(1, num(r, "Workgroup_Size_Y")) * max(1, num(r, "Workgroup_Size_Z")) for r in rs]
        grid = [num(r, "Grid_Size", "Grid_Size_X") * max(1, num(r, "Grid_Size_Y")) * max(1, num(r, "Grid_Size_Z")) for r in rs]
        if "Workgroup_Size" in rs[0]:   # the flat columns are already products
            wg = [num(r, "Workgroup_Size") for r in rs]
            grid = [num(r, "Grid_Size") for r in rs]
        wgs = [g // max(1, w) for g, w in zip(grid, wg)]
        waves = [k * -(-w // 64) for k, w in zip(wgs, wg)]
        a = alloc(n, rs[0])
        line = ("%-46s launches/batch %6.2f  workgroups median %7d max %7d  wg size %4d  us median %8.1f mean %8.1f  vgpr %3d agpr %3d alloc %3d  lds %6d scratch %4d"
                % (n[:46], len(rs) / batches, statistics.median(wgs), max(wgs), statistics.median(wg), statistics.median(d), statistics.mean(d),
                   regs(n, rs[0])[0], regs(n, rs[0])[1], a, num(rs[0], "LDS_Block_Size"), co[n][3] if n in co else num(rs[0], "Scratch_Size")))
        if a > room:
            slot_us = sum(w * t for w, t in zip(waves, d)) / batches   # wave-slot time per batch
            share = slot_us / (SIMDS * step_us)
            total_share += share
            line += "  | waves/batch %9.1f  wave-slot %10.0f wave-us per batch = %.4f of %d SIMDs x step (estimate)" % (sum(waves) / batches, slot_us, share, SIMDS)
        print(line)
    print("kernels that do not fit beside two waves of the pass: %.4f of the SIMDs' step time in sum (estimate, upper: every wave taken to live as long as its launch)" % total_share)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
