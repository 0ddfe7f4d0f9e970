"""What tools/orb_nms.sh left under its output folder (the text files of tools/orb_diet.sh's parts) as one JSON document on stdout:
the figures of profiles/orb_nms.json. A part that was not run is "not measured". Usage: python tools/orb_nms_summary.py OUT/orb_nms"""
import glob
import json
import os
import re
import statistics
import sys

out = sys.argv[1]
NOT = "not measured"


def lines(name):
    p = os.path.join(out, name)
    return open(p).read().splitlines() if os.path.exists(p) else None


def attribution():
    ls = lines("diet_attribution.txt")
    if ls is None:
        return NOT
    res = {}
    for l in ls:
        m = re.match(r"stages (\S+): (\{.*\})", l)
        if m:
            d = json.loads(m.group(2))
            r = res.setdefault(m.group(1), {"launch_ms": [], "value": []})
            r["launch_ms"].append(round(d["launch_ms"], 4)); r["value"].append(d["value"])
    for r in res.values():
        r["launch_ms_median"] = statistics.median(r["launch_ms"])
    if {"match", "orb,match", "match,verify"} <= set(res):
        res["orb_share_of_launch_ms"] = round(res["orb,match"]["launch_ms_median"] - res["match"]["launch_ms_median"], 4)
        res["verifier_share_of_launch_ms"] = round(res["match,verify"]["launch_ms_median"] - res["match"]["launch_ms_median"], 4)
    return res


def pmc():
    ls = lines("diet_pmc.txt")
    if ls is None:
        return NOT
    res = {}
    for l in ls:
        m = re.match(r"(\w+) (\S+)\s+SQ_INSTS_VALU (\S+) per launch, (\S+) per batch \((\d+) launches\)", l)
        if m:
            res.setdefault(m.group(1), {})[m.group(2)] = {"per_launch": float(m.group(3)), "per_batch": float(m.group(4)), "launches_per_batch": int(m.group(5)) // 23}
        m = re.match(r"(\w+) batch total (\S+)", l)
        if m:
            res.setdefault(m.group(1), {})["batch_total"] = float(m.group(2))
    if "parent" in res and "child" in res:
        p, c = res["parent"], res["child"]
        res["fast_nms_kernel child / parent"] = round(c["fast_nms_kernel"]["per_launch"] / p["fast_nms_kernel"]["per_launch"], 3)
        res["batch total removed"] = p["batch_total"] - c["batch_total"]
    return res


def trace():
    ls = lines("diet_trace.txt")
    if ls is None:
        return NOT
    res, which, n = {}, None, 0
    for l in ls:
        if l.startswith("== "):
            which, n = l[3:].strip(), 0
        m = re.match(r"\s+(\S+)\s+calls\s+\d+ avg\s+(\S+) us\s+per batch\s+(\S+) us", l)
        if m and which:
            res.setdefault("%s_%s" % (which, ("synth", "scenes")[min(n, 1)]), {})[m.group(1)] = {"avg_us": float(m.group(2)), "per_batch_us": float(m.group(3))}
        m = re.match(r"\s+sum per batch (\S+) us", l)
        if m and which:
            res["%s_%s" % (which, ("synth", "scenes")[min(n, 1)])]["sum_per_batch_us"] = float(m.group(1))
            n += 1
    return res


def batch():
    ls = lines("diet_batch.txt")
    if ls is None:
        return NOT
    res = {}
    for l in ls:
        m = re.match(r"batch (\w+): .*?: (\S+) ms per batch", l)
        if m:
            res.setdefault(m.group(1), []).append(float(m.group(2)))
    for k in list(res):
        res[k + "_median"] = statistics.median(res[k])
    if "parent" in res:
        res["parent_spread"] = round(max(res["parent"]) - min(res["parent"]), 4)
    return res


def bench_sessions():
    files = sorted(glob.glob(os.path.join(out, "diet_bench*.txt")))
    if not files:
        return NOT
    res = {}
    for i, f in enumerate(files):
        s = {}
        for l in open(f):
            m = re.match(r"bench (\w+): (\{.*\})", l)
            if m:
                d = json.loads(m.group(2))
                s.setdefault(m.group(1), []).append({"value": d["value"], "launch_ms": round(d["launch_ms"], 4), "stage_ms_per_step": d["stage_ms_per_step"]})
        for k in ("parent", "child"):
            if k in s:
                s[k + "_value_median"] = statistics.median(r["value"] for r in s[k])
                s[k + "_launch_ms_median"] = statistics.median(r["launch_ms"] for r in s[k])
        if "parent" in s and "child" in s:
            s["parent_value_max"] = max(r["value"] for r in s["parent"]); s["child_value_min"] = min(r["value"] for r in s["child"])
            s["verdict"] = "claimed" if s["child_value_min"] > s["parent_value_max"] else "not claimed"
        res["session_%d" % (i + 1)] = s
    return res


def full():
    ls = lines("diet_full.txt")
    if ls is None:
        return NOT
    return {m.group(1): json.loads(m.group(2)) for m in (re.match(r"full (\w+): (\{.*\})", l) for l in ls) if m}


dump = lines("diet_dump.txt")
print(json.dumps({"step0_attribution_on_parent": attribution(), "SQ_INSTS_VALU_per_launch": pmc(), "kernel_trace_one_batch_alone": trace(),
                  "batch_alone_ms": batch(), "headline": bench_sessions(), "same_results": dump[-1] if dump else NOT,
                  "full_extras_chained": full()}, indent=1))
