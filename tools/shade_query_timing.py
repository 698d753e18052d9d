"""What a radiance query costs beside the frame it could have been (rt_shade_rays_device against rt_time_render).

Per scene, one sample per pixel: the frame's own camera rays (rt_camera_rays_device, row-major) shaded as a
batch against the render kernel's time for the same frame on the same build -- the cost of leaving the tile
layout and reading rays from HBM; then the same rays shuffled, with and without RT_TRACE_SORT. Device event
times after a warm-up, the variants alternating, median of 5.

    python tools/shade_query_timing.py [--out FILE] [--scenes C3:1024,C4:512]
        writes profiles/shade_query_timing.json. DISTRAYTRACER_LIB picks another build of the library (the
        scheduler-flag experiment of DESIGN.md section 12: csrc/shade.hip compiled with render_minreg.hip's
        flags); --out keeps its numbers apart.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from distraytracer_old_amd import desc, rt, scenes  # noqa: E402

REPS = 5


def timed(fn, st, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(cfg, side, torch, dev, st):
    cli, _, _, _, seed = scenes.CONFIGS[cfg]
    n = side * side
    with rt.Scene.load_cli(cli, textures=scenes.prepare(cli)) as g:
        if g.info()["photon_mode"]:
            g.build_photons(seed)
        p = rt.params(side, side, 1, seed)
        cam = torch.zeros(n * desc.RAY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        g.camera_rays_device(p, cam.data_ptr(), sample=0, stream=st.cuda_stream)
        st.synchronize()
        perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).to(dev)
        shuf = cam.view(n, desc.RAY_DTYPE.itemsize)[perm].contiguous().view(-1)
        rgb = torch.zeros(n * 3, dtype=torch.float64, device=dev)
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

        def shade(rays, flags):
            g.shade_device(rays.data_ptr(), n, rgb.data_ptr(), status.data_ptr(), stream=st.cuda_stream, seed=seed, first_key=0,
                           sample=0, flags=flags)

        runs = {"camera": (cam, 0), "camera_sorted": (cam, rt.TRACE_SORT), "shuffled": (shuf, 0),
                "shuffled_sorted": (shuf, rt.TRACE_SORT)}
        for rays, fl in runs.values():  # warm-up (and the sort scratch's allocation)
            shade(rays, fl)
        st.synchronize()
        render_ms = [g.time_render(side, side, spp=1, seed=seed, warmup=2, iters=5)]
        ms = {k: [] for k in runs}
        for _ in range(REPS):
            for k, (rays, fl) in runs.items():
                ms[k].append(timed(lambda: shade(rays, fl), st, torch))
        render_ms.append(g.time_render(side, side, spp=1, seed=seed, warmup=2, iters=5))
        timed_mask = g.variant()[0]
    row = {"config": cfg, "scene": cli, "side": side, "rays": n, "spp": 1, "render_variant_mask": timed_mask,
           "render_kernel_ms": min(render_ms), "render_kernel_ms_all": render_ms}
    for k, v in ms.items():
        row[k + "_ms"] = statistics.median(v)
        row[k + "_ms_all"] = v
    row["camera_over_render"] = row["camera_ms"] / row["render_kernel_ms"]
    row["shuffled_sort_speedup"] = row["shuffled_ms"] / row["shuffled_sorted_ms"]
    print(f"{cfg} {side}^2: render {row['render_kernel_ms']:.3f} ms | shade camera {row['camera_ms']:.3f} "
          f"(sorted {row['camera_sorted_ms']:.3f}) | shuffled {row['shuffled_ms']:.3f} (sorted {row['shuffled_sorted_ms']:.3f})",
          flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "shade_query_timing.json"))
    ap.add_argument("--scenes", default="C3:1024,C4:512")
    a = ap.parse_args()
    import torch

    scenes.ensure_bun69k()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    table = []
    for item in a.scenes.split(","):
        cfg, side = item.split(":")
        table.append(measure(cfg, int(side), torch, dev, st))
    out = {"build_id": rt.build_id(), "lib": str(rt.lib_path().name), "reps": REPS, "device": torch.cuda.get_device_name(0),
           "table": table}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
