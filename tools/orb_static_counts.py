"""Static figures of orb.hip's kernels from the gfx950 assembly (hipcc -S, the Makefile's flags; no GPU needed): vector ALU, LDS and
vector memory instructions in each kernel's text, registers, LDS bytes, scratch bytes -- the columns of profiles/orb_diet.json.
Usage: python tools/orb_static_counts.py [path to orb.hip] [kernel ...]"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tod_amd", "csrc", "orb.hip")
want = sys.argv[2:] or ["resize_kernel", "fast_nms_kernel", "describe_kernel"]
with tempfile.TemporaryDirectory() as d:
    out = os.path.join(d, "orb.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                    "-o", out, src], check=True, stderr=subprocess.DEVNULL)
    asm = open(out).read()
res = {}
for name in want:
    m = re.search(r"^(_Z\S*%s\S*):[^\n]*\n(.*?)\n\.Lfunc_end" % name, asm, re.S | re.M)
    ins = [l.split(";")[0].strip().split()[0] for l in m.group(2).split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    meta = next(e for e in re.split(r"\n  - ", asm[asm.index("amdhsa.kernels:"):]) if re.search(r"\.name:\s+%s\b" % re.escape(m.group(1)), e))
    field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))
    res[name] = {"valu": sum(i.startswith("v_") for i in ins), "lds": sum(i.startswith("ds_") for i in ins),
                 "vmem": sum(i.startswith(("global_", "buffer_", "flat_", "scratch_")) for i in ins),
                 "vgpr": field("vgpr_count"), "lds_bytes": field("group_segment_fixed_size"), "scratch": field("private_segment_fixed_size")}
print(json.dumps(res, indent=1))
