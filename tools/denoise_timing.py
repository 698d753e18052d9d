"""What the denoise step costs beside one more sample (rt_denoise_run_device and rt_denoise_create against
rt_accum_add(1)).

Per scene and size, on an accumulator that holds 4 samples: a run with the defaults for levels = 0 .. 5 (init and
output alone, then one more a-trous level each: the differences are the per-level times), and add(1) of the same
frame, alternating within one run on one caller's stream; device event times after a warm-up of every shape, median
of 5. The guide build (rt_denoise_create: camera rays, the trace, the pack) blocks, so it is timed by the wall clock
around create and destroy, median of 5 after one warm-up. Per level the filter must move 64 bytes in and 32 bytes out
per pixel (its own record of the plane, the two guide records, the new record; the 24 neighbours' records are
re-reads the caches can serve): those bytes over the measured time, as a fraction of the HBM3E peak (8.0 TB/s by
its specification, 6.29 TB/s as a float4 copy achieves it).

    python tools/denoise_timing.py [--out FILE] [--scenes C3:1024,C4:2048]
        writes profiles/denoise_timing.json and prints the table of DESIGN.md section 17.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from distraytracer_old_amd import rt, scenes  # noqa: E402

REPS = 5
SAMPLES = 4
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29
LEVEL_BYTES_PER_PIXEL = 64 + 32


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
    defaults = rt.DenoiseParams.defaults()
    rgb = torch.zeros((side, side, 3), dtype=torch.float32, device=dev)
    argb = torch.zeros((side, side), dtype=torch.int32, device=dev)
    with rt.Scene.load_cli(cli, textures=scenes.prepare(cli)) as g:
        if g.info()["photon_mode"]:
            g.build_photons(seed)
        with g.accumulator(side, side, seed=seed, moments=True) as a:
            a.add(SAMPLES, stream=st.cuda_stream)
            st.synchronize()
            build = []
            for r in range(REPS + 1):
                t0 = time.perf_counter()
                d = a.denoiser()
                t1 = time.perf_counter()
                d.close()
                if r:  # the first round is the warm-up
                    build.append(1e3 * (t1 - t0))
            with a.denoiser() as d:
                runs = {f"run_levels_{L}": (lambda L: lambda: d.run_device(rgb.data_ptr(), argb.data_ptr(), stream=st.cuda_stream, levels=L))(L)
                        for L in range(defaults.levels + 1)}
                runs["add_1"] = lambda: a.add(1, stream=st.cuda_stream)
                for fn in runs.values():  # warm-up of every shape
                    fn()
                st.synchronize()
                ms = {k: [] for k in runs}
                for r in range(REPS):
                    for k, fn in runs.items():
                        ms[k].append(timed(fn, st, torch))
                st.synchronize()
    med = {k: statistics.median(v) for k, v in ms.items()}
    full = med[f"run_levels_{defaults.levels}"]
    levels = []
    for L in range(1, defaults.levels + 1):
        t = med[f"run_levels_{L}"] - med[f"run_levels_{L - 1}"]
        tbs = LEVEL_BYTES_PER_PIXEL * n / (t * 1e-3) / 1e12 if t > 0 else None
        levels.append({"level": L - 1, "stride": 1 << (L - 1), "ms": t, "unique_TB_per_s": tbs,
                       "of_hbm_spec_peak": tbs / HBM_SPEC_TBS if tbs else None, "of_hbm_copy_rate": tbs / HBM_COPY_TBS if tbs else None})
    row = {"config": cfg, "scene": cli, "side": side, "pixels": n, "samples_held": SAMPLES,
           "params": {"levels": defaults.levels, "normal_log2": defaults.normal_log2, "sigma_l": defaults.sigma_l, "sigma_z": defaults.sigma_z},
           "run_ms": full, "run_ms_all": ms[f"run_levels_{defaults.levels}"],
           "run_spread": (max(ms[f"run_levels_{defaults.levels}"]) - min(ms[f"run_levels_{defaults.levels}"])) / full,
           "init_and_output_ms": med["run_levels_0"], "levels": levels, "ms_by_levels": {k: v for k, v in ms.items() if k != "add_1"},
           "guide_build_wall_ms": statistics.median(build), "guide_build_wall_ms_all": build,
           "add_1_ms": med["add_1"], "add_1_ms_all": ms["add_1"], "run_over_add_1": full / med["add_1"],
           "guide_build_over_add_1": statistics.median(build) / med["add_1"],
           "unique_bytes_per_level": LEVEL_BYTES_PER_PIXEL * n}
    print(f"{cfg} {side}^2: run {full:.3f} ms (spread {100 * row['run_spread']:.1f} %), init+output {med['run_levels_0']:.3f} ms, levels " +
          ", ".join(f"{v['ms']:.3f}" for v in levels) + f" ms | guide build {row['guide_build_wall_ms']:.3f} ms (wall) | add(1) "
          f"{med['add_1']:.3f} ms | run / add(1) {row['run_over_add_1']:.3f}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "denoise_timing.json"))
    ap.add_argument("--scenes", default="C3:1024,C4:2048")
    a = ap.parse_args()
    import torch

    scenes.ensure_bun69k()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)  # not the null stream: the adds read NULL as the scene's own stream
    table = []
    for item in a.scenes.split(","):
        cfg, side = item.split(":")
        table.append(measure(cfg, int(side), torch, dev, st))
    out = {"build_id": rt.build_id(), "lib": str(rt.lib_path().name), "reps": REPS, "device": torch.cuda.get_device_name(0),
           "hbm_peak_TB_per_s": {"specification": HBM_SPEC_TBS, "float4_copy": HBM_COPY_TBS}, "table": table}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("| config | run ms | per level ms | worst level, of 8.0 TB/s | guide build ms (wall) | add(1) ms | run / add(1) |")
    for r in table:
        worst = max(r["levels"], key=lambda v: v["ms"])
        print(f"| {r['config']} {r['side']}^2 | {r['run_ms']:.3f} | " + " ".join(f"{v['ms']:.3f}" for v in r["levels"]) +
              f" | {100 * (worst['of_hbm_spec_peak'] or 0):.1f} % | {r['guide_build_wall_ms']:.2f} | {r['add_1_ms']:.3f} | {r['run_over_add_1']:.3f} |")


if __name__ == "__main__":
    main()
