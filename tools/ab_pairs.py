#!/usr/bin/env python3
"""Same-box A/B of two builds of the library: parent and new alternating, a warm-up pair and then
`--pairs` measured pairs, one subprocess per run (the bar of a render-kernel change).

  python tools/ab_pairs.py --parent tools/_ab/lib_parent.so [--new <lib>] [--pairs 3] [--cfgs C4,C5]

Per run: bench.py's C3 line (ms_per_step, roofline.kernel_ms, build id) and, per --cfgs entry,
tools/variant_sweep.py's frame time and ARGB hash. Every line is printed as it is measured; the last line is
the JSON summary: the runs, the parent's max - min, and gain_min = fastest parent - slowest new.
clears_bar: every new run faster than every parent run by at least three times the parent's spread;
not_slower_beyond_spread: the slowest new run is no slower than the slowest parent run plus that spread.
A run that fails or times out ends the script (nothing more is started on the GPU)."""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]


def run(cmd, lib, limit):
    env = dict(os.environ)
    if lib:
        env["DISTRAYTRACER_LIB"] = str(Path(lib).resolve())
    else:
        env.pop("DISTRAYTRACER_LIB", None)
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0 or not r.stdout.strip():
        print("FAILED", cmd, r.returncode, r.stderr[-2000:], flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default="", help="default: the in-tree library")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--cfgs", default="C4,C5")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    cfgs = [c for c in a.cfgs.split(",") if c]
    res = {}
    for p in range(a.pairs + 1):
        for side, lib in (("parent", a.parent), ("new", a.new)):
            tag = "warmup" if p == 0 else ""
            b = run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)], lib, 300)
            vals = {"c3_ms_per_step": b["ms_per_step"], "c3_kernel_ms": b.get("roofline", {}).get("kernel_ms"),
                    "c3_build": b.get("build_id") or b.get("build", {}).get("id")}
            for c in cfgs:
                v = run([sys.executable, "tools/variant_sweep.py", "one", "--cfg", c], lib, 300)
                vals[f"{c.lower()}_ms"], vals[f"{c.lower()}_hash"] = v["ms"], v["hash"]
            for k, v in vals.items():
                print(k, side, tag, v, flush=True)
                if p > 0:
                    res.setdefault(k, {"parent": [], "new": []})[side].append(v)
    for k, r in res.items():
        if k.endswith("_ms") or k.endswith("ms_per_step"):
            sp = max(r["parent"]) - min(r["parent"])
            r["parent_spread"] = sp
            r["gain_min"] = min(r["parent"]) - max(r["new"])
            r["clears_bar"] = r["gain_min"] >= 3 * sp and r["gain_min"] > 0
            r["not_slower_beyond_spread"] = max(r["new"]) <= max(r["parent"]) + sp
    print(json.dumps(res))


if __name__ == "__main__":
    main()
