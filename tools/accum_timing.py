"""What progressive accumulation costs beside the frame rendered in one go (rt_accum_add against rt_time_render).

Per scene, 16 samples per pixel in total: the render kernel's time for the 16-spp frame (the yardstick, the same
build, the same run); one add(16), which runs the render's wave layout and beyond it only reads and writes the
carried sums; the chunkings 2 x 8, 4 x 4 and 16 x 1 (less coherent waves, one launch per chunk); and what a host
had before -- rt_camera_rays_device plus rt_shade_rays_device per sample, the colours left in HBM for a fold
that is not timed. Device event times after a warm-up of every shape, the variants alternating within one run,
median of 5; the render is timed before, between and after, and the spread of those timings is reported beside
the add(16) it is compared with. The render is also timed with RT_RENDER_ROWMAJOR: add dispatches its tiles
row-major, without the render's longest-first schedule, so that figure separates the dispatch order from the kernel.

--pose adds the camera pose (rt_accum_set_camera): add(16), without and with moments, of an accumulator that looks
through a small look-at move, alternating with the un-posed add(16) of the same build in the same repetitions. The
posed kernel is reported over the un-posed one, beside the un-posed one's own run-to-run spread. The moved eye sees
another picture, so that ratio is of two frames; add(16) through the identity pose, which shoots the un-posed
frame's own rays, is timed too and is the ratio of the two kernels on the same work.

    python tools/accum_timing.py [--out FILE] [--scenes C3:1024,C4:512,C5:256] [--pose]
        writes profiles/accum_timing.json.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from distraytracer_old_amd import desc, rt, scenes  # noqa: E402

REPS = 5
TOTAL = 16
CHUNKINGS = {"add_16": [16], "add_2x8": [8, 8], "add_4x4": [4] * 4, "add_16x1": [1] * 16}
POSE_EYE, POSE_AT = (0.3, 0.2, 0.5), (0.0, 0.0, -4.0)  # the scenes stay in view


def timed(fn, st, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(cfg, side, torch, dev, st, pose=False):
    cli, _, _, _, seed = scenes.CONFIGS[cfg]
    n = side * side
    with rt.Scene.load_cli(cli, textures=scenes.prepare(cli)) as g:
        if g.info()["photon_mode"]:
            g.build_photons(seed)
        p = rt.params(side, side, TOTAL, seed)
        cam = torch.zeros(n * desc.RAY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        rgb = torch.zeros(n * 3, dtype=torch.float64, device=dev)
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

        def render(flags=0):
            return g.time_render(side, side, spp=TOTAL, seed=seed, warmup=2, iters=5, flags=flags)

        def queries():  # the route of DESIGN.md section 12: per sample the camera rays as data, then the shading tree on them
            for s in range(TOTAL):
                g.camera_rays_device(p, cam.data_ptr(), sample=s, stream=st.cuda_stream)
                g.shade_device(cam.data_ptr(), n, rgb.data_ptr(), status.data_ptr(), stream=st.cuda_stream, seed=seed,
                               first_key=0, sample=s)

        with g.accumulator(side, side, seed=seed) as acc, g.accumulator(side, side, seed=seed, moments=True) as accm:
            def adds(a, chunks):
                def run():
                    for c in chunks:  # samples done, done + 1, ...: later samples, the same work
                        a.add(c, stream=st.cuda_stream)
                return run

            runs = {k: adds(acc, c) for k, c in CHUNKINGS.items()}
            runs["add_16_moments"] = adds(accm, [TOTAL])
            runs["queries_16"] = queries
            posed = []
            if pose:
                M = rt.look_at(POSE_EYE, POSE_AT)
                posed = [g.accumulator(side, side, seed=seed, pose=M), g.accumulator(side, side, seed=seed, moments=True, pose=M)]
                runs["add_16_pose"] = adds(posed[0], [TOTAL])
                runs["add_16_moments_pose"] = adds(posed[1], [TOTAL])
                # the identity: the un-posed frame's own rays (up to the sign of a zero), so the same work per wave
                posed.append(g.accumulator(side, side, seed=seed, pose=[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))
                runs["add_16_identity_pose"] = adds(posed[2], [TOTAL])
            for fn in runs.values():  # warm-up of every shape
                fn()
            st.synchronize()
            render_ms = [render()]
            rowmajor_ms = [render(rt.RENDER_ROWMAJOR)]  # the render without its longest-first tile schedule, as add dispatches
            ms = {k: [] for k in runs}
            for r in range(REPS):
                for k, fn in runs.items():
                    ms[k].append(timed(fn, st, torch))
                render_ms.append(render())
                rowmajor_ms.append(render(rt.RENDER_ROWMAJOR))
            st.synchronize()
            for a in posed:
                a.close()
        timed_mask = g.variant()[0]
    row = {"config": cfg, "scene": cli, "side": side, "pixels": n, "samples": TOTAL, "render_variant_mask": timed_mask,
           "render_kernel_ms": statistics.median(render_ms), "render_kernel_ms_all": render_ms,
           "render_spread": (max(render_ms) - min(render_ms)) / statistics.median(render_ms),
           "render_rowmajor_ms": statistics.median(rowmajor_ms), "render_rowmajor_ms_all": rowmajor_ms}
    row["add_16_over_render_rowmajor"] = statistics.median(ms["add_16"]) / row["render_rowmajor_ms"]
    for k, v in ms.items():
        row[k + "_ms"] = statistics.median(v)
        row[k + "_ms_all"] = v
        row[k + "_over_render"] = row[k + "_ms"] / row["render_kernel_ms"]
    if pose:  # the posed kernel over its un-posed twin, and how far the twin's own repetitions lie apart
        for k in ("add_16", "add_16_moments"):
            row[k + "_spread"] = (max(ms[k]) - min(ms[k])) / row[k + "_ms"]
            row[k + "_pose_over_" + k] = row[k + "_pose_ms"] / row[k + "_ms"]
        row["add_16_identity_pose_over_add_16"] = row["add_16_identity_pose_ms"] / row["add_16_ms"]
        row["pose"] = {"eye": POSE_EYE, "at": POSE_AT}
    print(f"{cfg} {side}^2 x {TOTAL}: render {row['render_kernel_ms']:.3f} ms (spread {100 * row['render_spread']:.1f} %), row-major "
          f"{row['render_rowmajor_ms']:.3f} | " +
          " | ".join(f"{k} {row[k + '_ms']:.3f}" for k in ms), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "accum_timing.json"))
    ap.add_argument("--scenes", default="C3:1024,C4:512,C5:256")
    ap.add_argument("--pose", action="store_true", help="also time add(16) through a camera pose")
    a = ap.parse_args()
    import torch

    scenes.ensure_bun69k()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)  # not the null stream: rt_accum_add reads NULL as the scene's own stream
    table = []
    for item in a.scenes.split(","):
        cfg, side = item.split(":")
        table.append(measure(cfg, int(side), torch, dev, st, a.pose))
    out = {"build_id": rt.build_id(), "lib": str(rt.lib_path().name), "reps": REPS, "device": torch.cuda.get_device_name(0),
           "table": table}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
