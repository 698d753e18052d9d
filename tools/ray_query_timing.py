"""Ray-query throughput on the C3 scene (rt_trace_rays_device): Mray/s of 2^22 rays for
{packet, lanes} x {camera order, shuffled} x {closest, any}, timed with device events after a warm-up,
median of 5; the render kernel's own rate on C3 beside it for scale. The table tells a caller when to
pass RT_TRACE_LANES: a packet walks the union of its 64 rays' paths, which pays for coherent batches
and may not for incoherent ones. Writes profiles/ray_query_timing.json tagged with rt_build_id().

    python tools/ray_query_timing.py [--out FILE] [--log2n 22]
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from distraytracer_old_amd import desc, rt, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "ray_query_timing.json"))
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    cli, W, H, spp, seed = scenes.CONFIGS["C3"]
    side = 1 << (a.log2n // 2)
    n = side * side
    # camera order: the un-jittered camera rays of a side x side frame, row-major (fov 60)
    view_z = -1 * (side / 2.0) / math.tan((math.pi * 60.0 / 180.0) / 2)
    col, row = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64))
    d = np.stack([col - side / 2.0, -1 * (row - side / 2.0), np.full((side, side), view_z)], -1).reshape(-1, 3)
    rays = rt.rays(np.zeros_like(d), d, np.inf)
    perm = np.random.default_rng(1).permutation(n)
    dev = torch.device("cuda", 0)
    orders = {"camera": torch.from_numpy(rays.view(np.uint8).reshape(-1)).to(dev),
              "shuffled": torch.from_numpy(rays[perm].view(np.uint8).reshape(-1)).to(dev)}
    hits = torch.zeros(n * desc.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    occ = torch.zeros(n, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev)
    table = []
    with rt.Scene.load_cli(cli) as g:
        for trav, tf in (("packet", 0), ("lanes", rt.TRACE_LANES)):
            for order, t_rays in orders.items():
                for query, qf in (("closest", 0), ("any", rt.TRACE_ANY)):
                    def go():
                        g.trace_device(t_rays.data_ptr(), n, hits_ptr=0 if qf else hits.data_ptr(),
                                       occ_ptr=occ.data_ptr() if qf else 0, stream=st.cuda_stream, flags=tf | qf)
                    go()  # warm-up
                    st.synchronize()
                    ms = []
                    for _ in range(a.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        go()
                        e1.record(st)
                        e1.synchronize()
                        ms.append(e0.elapsed_time(e1))
                    med = statistics.median(ms)
                    share = float((occ == 1).float().mean()) if qf else \
                        float((hits.view(-1, desc.HIT_DTYPE.itemsize)[:, 72] & 1).float().mean())
                    table.append({"traversal": trav, "order": order, "query": query, "ms": med, "ms_all": ms,
                                  "mray_per_s": n / med / 1e3, "hit_share": share})
                    print(f"{trav:7s} {order:9s} {query:8s} {med:9.3f} ms  {n / med / 1e3:9.1f} Mray/s  share {share:.3f}")
        # the render kernel on C3 for scale: every ray it traces (camera, shadow, reflection, refraction)
        ms = g.time_render(W, H, spp=spp, seed=seed, warmup=2, iters=5)
        _, _, stc = g.render_count(W, H, spp=spp, seed=seed)
        nr = stc["camera"] + stc["shadow"] + stc["refl"] + stc["refr"]
        render = {"config": "C3", "ms": ms, "rays": int(nr), "gray_per_s": nr / ms / 1e6,
                  "camera_msample_per_s": W * H * spp / ms / 1e3}
        print(f"render C3: {ms:.3f} ms, {nr} rays, {render['gray_per_s']:.3f} Gray/s")
    out = {"build_id": rt.build_id(), "scene": cli, "rays": n, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "table": table, "render": render}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
