#!/usr/bin/env python3
"""Kernel tuning sweep: build the library with different compile-time settings
(here, on CPU) and time each on the GPU box, one subprocess per build.

  python tools/variant_sweep.py build            # -> tools/_variants/*.so
  python tools/variant_sweep.py run [--cfg C3]   # on the GPU: ms/frame + ARGB hash per build

Every build must give the same ARGB hash (the specialisations change speed, not results), the
profiling builds (RT_PROF_*) excepted. Every define below names a macro that csrc/ reads
(tests/test_variant_table.py); switches whose A/B is settled are folded into the code and listed in
DESIGN.md "Retired switches".
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
OUT = REPO / "tools" / "_variants"
VARIANTS = {  # name -> -D defines; names like "s12w4" are parsed (see defines_of)
    "noshadow": ["RT_PROF_NOSHADOW"],          # profiling only: results differ
    "nosec": ["RT_PROF_NOSECONDARY"],
    "primary": ["RT_PROF_NOSHADOW", "RT_PROF_NOSECONDARY"],
    "nogather": ["RT_PROF_NOGATHER"],
    "nophong": ["RT_PROF_NOPHONG"],
    "notex": ["RT_PROF_NOTEX"],                # object textures -> plain diffuse
    "noshade": ["RT_PROF_NOSHADE"],            # camera rays traced, no hit record / shading
    "notrace": ["RT_PROF_NOTRACE"],            # camera rays generated, nothing traced
    "wprio": ["-Xarch_device", "-mllvm=--amdgpu-set-wave-priority"],  # compiler flags (results equal)
    "itsched": ["-Xarch_device", "-mllvm=--amdgpu-sched-strategy=gcn-iterative-max-occupancy-experimental"],
    "bias0": ["-Xarch_device", "-mllvm=--amdgpu-schedule-metric-bias=0"],
    "trk": ["-Xarch_device", "-mllvm=--amdgpu-use-amdgpu-trackers=1"],
    # scheduler of trace.hip only (C4's variant and the others; C3 / C5 are in render_minreg.hip)
    "mrnohrp": ["@render_minreg.hip:-Xarch_device", "@render_minreg.hip:-mllvm=--amdgpu-disable-unclustered-high-rp-reschedule=1"],
    "mrbias0": ["@render_minreg.hip:-Xarch_device", "@render_minreg.hip:-mllvm=--amdgpu-schedule-metric-bias=0"],
    "c4ilp": ["@trace.hip:-Xarch_device", "@trace.hip:-mllvm=--amdgpu-sched-strategy=max-ilp"],
    "c4mmc": ["@trace.hip:-Xarch_device", "@trace.hip:-mllvm=--amdgpu-sched-strategy=max-memory-clause"],
    "c4itilp": ["@trace.hip:-Xarch_device", "@trace.hip:-mllvm=--amdgpu-sched-strategy=iterative-ilp"],
    "minreg": ["-Xarch_device", "-mllvm=--amdgpu-sched-strategy=iterative-minreg"],
    "trkminreg": ["-Xarch_device", "-mllvm=--amdgpu-use-amdgpu-trackers=1", "-Xarch_device",
                  "-mllvm=--amdgpu-sched-strategy=iterative-minreg"],
    # photon gather: sizes and thresholds (defaults: EDGES 16, SHELL 10, START 1.15, DIV_FRAC 2, DIV_R 2.0,
    # PH_BATCH 1, PH_VLOAD 1)
    "ed32": ["RT_KNN_EDGES=32"],               # u32 buckets of the last-resort counting pass
    "sh12": ["RT_KNN_SHELL=12"],               # window list in LDS: up to 12 photons
    "h32b2": ["RT_KNN_EDGES=32", "RT_PH_BATCH=2"],
    "h32sh12": ["RT_KNN_EDGES=32", "RT_KNN_SHELL=12"],
    "vl2": ["RT_PH_VLOAD=2"],                  # leaf photons (vector load + v_readlane): two independent distances per step
    "vl4": ["RT_PH_VLOAD=4"],
    "st10": ["RT_KNN_START=1.0"],              # the start window: x the d^2 holding K photons at the node's density
    "st11": ["RT_KNN_START=1.1"],
    "st12": ["RT_KNN_START=1.2"],
    "st125": ["RT_KNN_START=1.25"],
    "st13": ["RT_KNN_START=1.3"],
    "kdf4": ["RT_KNN_DIV_FRAC=4"],             # lane-by-lane scans when 1/4 (1/1) of a call's lanes are far apart
    "kdf1": ["RT_KNN_DIV_FRAC=1"],
    "kdr4": ["RT_KNN_DIV_R=4.0"],              # ... farther than 4 (1) start radii from the first lane's point
    "kdr1": ["RT_KNN_DIV_R=1.0"],
    "tl": ["RT_PROF_TIMELINE"],               # workgroup timeline (tools/timeline.py)
    "pkstat": ["RT_PROF_PKSTAT"],             # packet lane utilisation (tools/pkstat.py)
    "shnoquad": ["RT_PROF_SH_NOQUAD"],         # shadow scan without quads / planes
    "shnoimpl": ["RT_PROF_SH_NOIMPL"],         # shadow scan without implicit primitives
    "shnoaccel": ["RT_PROF_SH_NOACCEL"],       # shadow scan without BVHs / lists
    "shscan": ["RT_PROF_SH_SCANONLY"],         # shadow rays: the top-level scan only, no tests
    "regions": ["RT_PROF_REGIONS"],           # wave time per region (tools/regions.py)
    "base": [],                                # the default build
    "wf5": ["RT_WF_WAVES=5"],                  # level-synchronous kernels at 5 / 3 waves per SIMD
    "wf3": ["RT_WF_WAVES=3"],
    "nosample": ["RT_PROF_NOSAMPLE"],         # camera setup, sums and output alone (results differ)
    # known normalisations: each part off, and all four off (the statements as they were)
    "ru0": ["RT_RENORM_UNIT=0"], "dw0": ["RT_HIT_DW=0"], "ld0": ["RT_LIGHT_DIST=0"], "ps0": ["RT_PLANAR_SIGN=0"],
    "kn0": ["RT_RENORM_UNIT=0", "RT_HIT_DW=0", "RT_LIGHT_DIST=0", "RT_PLANAR_SIGN=0"],
    "hn0": ["RT_HIT_NRM=0"],                  # hit normals computed per hit, not read from the upload-time table
    "wr0": ["RT_WREC=0"],                     # NodeF / TriF / TriD geometry as field loads, not whole-record loads
    "c4mr": ["@trace.hip:-Xarch_device", "@trace.hip:-mllvm=--amdgpu-sched-strategy=iterative-minreg",
             "@trace.hip:-Xarch_device", "@trace.hip:-mllvm=--amdgpu-use-amdgpu-trackers=1"],
}
FIELDS = {"w": "RT_RENDER_WAVES", "s": "RT_STACK_LDS", "g": "RT_MAX_G", "l": "RT_PK_LDS", "b": "RT_PH_BATCH"}


def defines_of(name: str) -> list[str]:
    import re
    if name in VARIANTS:
        return VARIANTS[name]
    return [f"{FIELDS[k]}={v}" for k, v in re.findall(r"([a-z])(\d+)", name)]


def _build_one(n):
    from distraytracer_old_amd import build
    p = build.build(defines=defines_of(n), out=OUT / f"lib_{n}.so")
    for o in OUT.glob(f"lib_{n}.*.o"):
        o.unlink()
    return p


def do_build(names):
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=4) as ex:
        for p in ex.map(_build_one, names):
            print("built", p, flush=True)


def time_one(cfg: str, W: int, H: int, spp: int, iters: int, flags: int, save: str = ""):
    from distraytracer_old_amd import rt, scenes
    cli, W0, H0, spp0, seed = scenes.CONFIGS[cfg]
    scenes.ensure_bun69k()
    with rt.Scene.load_cli(cli, textures=scenes.prepare(cli)) as s:
        W = W or W0; H = H or H0; spp = spp or spp0
        rgb, argb = s.render(W, H, spp=spp, seed=seed, flags=flags)
        if save:  # the frame, to compare builds whose images may differ in the last bits
            import numpy as np
            np.savez_compressed(save, rgb=rgb, argb=argb)
        ms = s.time_render(W, H, spp=spp, seed=seed, warmup=1, iters=iters, flags=flags)
    return {"ms": ms, "hash": hashlib.sha1(argb.tobytes()).hexdigest()[:12], "W": W, "H": H, "spp": spp}


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["build", "run", "one"])
    ap.add_argument("--cfg", default="C3")
    ap.add_argument("--names", default="w4,w5")
    ap.add_argument("--W", type=int, default=0)
    ap.add_argument("--H", type=int, default=0)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--dir", default="", help="run: where the built libraries are (default tools/_variants)")
    ap.add_argument("--save", default="", help="directory: each build's frame as <name>_<cfg>.npz")
    a = ap.parse_args()
    names = a.names.split(",")
    if a.mode == "build":
        do_build(names)
    elif a.mode == "one":
        print(json.dumps(time_one(a.cfg, a.W, a.H, a.spp, a.iters, a.flags, a.save)))
    else:
        for n in names:
            lib = (Path(a.dir) if a.dir else OUT) / f"lib_{n}.so"
            env = dict(os.environ, DISTRAYTRACER_LIB=str(lib))
            cmd = [sys.executable, __file__, "one", "--cfg", a.cfg, "--W", str(a.W), "--H", str(a.H), "--spp", str(a.spp),
                   "--iters", str(a.iters), "--flags", str(a.flags)]
            if a.save:
                os.makedirs(a.save, exist_ok=True)
                cmd += ["--save", os.path.join(a.save, f"{n}_{a.cfg}.npz")]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            line = r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else r.stderr[-800:]
            print(n, a.cfg, line, flush=True)
            if r.returncode != 0:
                sys.exit(r.returncode)


if __name__ == "__main__":
    main()
