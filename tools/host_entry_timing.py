"""What the blocking host-buffer entries cost on the C3 scene with the 2^20 camera rays of a 1024 x 1024 frame
(four staging chunks of 2^18 rays): rt_camera_rays, rt_trace_rays, rt_trace_order, rt_shade_rays, and rt_render
at 1 spp. One warm-up call, then 9 timed calls each with the host clock (every entry ends in a stream wait):
median, min and max in ms. Prints one JSON line with the times, the library's build id and a hash of every
output, so two builds (DISTRAYTRACER_LIB) can be compared for speed and for bytes.

    python tools/host_entry_timing.py
"""
import hashlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from distraytracer_old_amd import rt, scenes  # noqa: E402

REPS = 9
W = H = 1024


def timed(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def h(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def main():
    import torch

    assert torch.cuda.is_available()
    cli = scenes.CONFIGS["C3"][0]
    scenes.ensure_bun69k()
    out = {"build": rt.build_id() if hasattr(rt, "build_id") else None}
    with rt.Scene.load_cli(cli, textures=scenes.prepare(cli), device=0) as s:
        keep = {}
        out["rt_camera_rays"] = timed(lambda: keep.__setitem__("rays", s.camera_rays(W, H, spp=1)))
        r = keep["rays"]
        o, d = r["o"], r["d"]
        out["rt_trace_rays"] = timed(lambda: keep.__setitem__("hits", s.trace(o, d)))
        out["rt_trace_order"] = timed(lambda: keep.__setitem__("order", s.trace_order(o, d)))
        out["rt_shade_rays"] = timed(lambda: keep.__setitem__("rgb", s.shade(o, d, seed=0x5EED0001)))
        out["rt_render_1spp"] = timed(lambda: keep.__setitem__("frame", s.render(W, H, spp=1)))
        out["hash"] = {"rays": h(r), "hits": h(keep["hits"]), "order": h(keep["order"]), "rgb": h(keep["rgb"][0]),
                       "status": h(keep["rgb"][1]), "argb": h(keep["frame"][1])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
