"""What the selective add costs beside the whole-frame add (rt_accum_add_selected against rt_accum_add).

Per scene, 16 samples per selected pixel: add(16) on an accumulator without counts (the yardstick: the existing
tile kernel, the same build, the same run); add_selected(16) with every pixel selected (the cost of the list
indirection and the Morton layout); then 50 %, 25 % and 5 % of the pixels selected in two ways -- as whole 8 x 8
tiles (dense: a wave's pixels are neighbours) and as a per-pixel random mask (scattered: they are not, and the
packet traversal loses its coherence). Reported per case: ms, and ms per selected pixel relative to the whole
frame's add(16). The selection itself (select_error, select_mask_device) is timed by the wall clock, since those
entries block. Device event times after a warm-up of every shape, the variants alternating within one run, median
of 5.

    python tools/adaptive_timing.py [--out FILE] [--scenes C3:1024,C4:512,C5:256]
        writes profiles/adaptive_timing.json and prints the table of DESIGN.md section 16.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

from distraytracer_old_amd import rt, scenes  # noqa: E402

REPS = 5
COUNT = 16
FRACTIONS = (0.5, 0.25, 0.05)


def timed(fn, st, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def masks(side, rng):
    """name -> bool [side, side]: every pixel, then each fraction as whole tiles and as single pixels"""
    out = {"all": np.ones((side, side), dtype=bool)}
    t = (side + 7) // 8
    for f in FRACTIONS:
        tiles = rng.random((t, t)) < f
        out[f"dense_{int(100 * f)}"] = np.kron(tiles, np.ones((8, 8), dtype=bool))[:side, :side].astype(bool)
        out[f"scattered_{int(100 * f)}"] = rng.random((side, side)) < f
    return out


def measure(cfg, side, torch, dev, st):
    cli, _, _, _, seed = scenes.CONFIGS[cfg]
    n = side * side
    rng = np.random.default_rng(1234)
    with rt.Scene.load_cli(cli, textures=scenes.prepare(cli)) as g:
        if g.info()["photon_mode"]:
            g.build_photons(seed)
        ms_of = masks(side, rng)
        with g.accumulator(side, side, seed=seed, moments=True) as whole:
            accs = {k: g.accumulator(side, side, seed=seed, moments=True, counts=True) for k in ms_of}
            try:
                picked = {k: accs[k].select_mask(m) for k, m in ms_of.items()}
                runs = {"add_16": lambda: whole.add(COUNT, stream=st.cuda_stream)}
                for k in ms_of:
                    runs["selected_" + k] = (lambda a: lambda: a.add_selected(COUNT, stream=st.cuda_stream))(accs[k])
                for fn in runs.values():  # warm-up of every shape
                    fn()
                st.synchronize()
                ms = {k: [] for k in runs}
                for r in range(REPS):
                    for k, fn in runs.items():  # later samples of the same pixels: the same work
                        ms[k].append(timed(fn, st, torch))
                st.synchronize()
                # the selection entries block: wall clock, on the accumulator that has its 32+ samples everywhere
                a = accs["all"]
                err = a.error()
                thr = float(np.median(err[np.isfinite(err)]))
                dmask = torch.from_numpy(ms_of["scattered_25"].astype(np.uint8)).to(dev)
                torch.cuda.synchronize(dev)
                sel = {"select_error": [], "select_mask_device": []}
                for r in range(REPS + 1):
                    t0 = time.perf_counter()
                    n_err = a.select_error(thr, 1 << 30)
                    t1 = time.perf_counter()
                    a.select_mask_device(dmask.data_ptr(), stream=st.cuda_stream)
                    t2 = time.perf_counter()
                    if r:  # the first round is the warm-up
                        sel["select_error"].append(1e3 * (t1 - t0))
                        sel["select_mask_device"].append(1e3 * (t2 - t1))
            finally:
                for a in accs.values():
                    a.close()
        timed_mask = g.variant()[0]
    row = {"config": cfg, "scene": cli, "side": side, "pixels": n, "samples_per_selected_pixel": COUNT, "render_variant_mask": timed_mask,
           "add_16_ms": statistics.median(ms["add_16"]), "add_16_ms_all": ms["add_16"],
           "add_16_spread": (max(ms["add_16"]) - min(ms["add_16"])) / statistics.median(ms["add_16"]),
           "select_error_selected": n_err, "cases": []}
    per_px = row["add_16_ms"] / n
    for k in ms_of:
        v = ms["selected_" + k]
        med = statistics.median(v)
        row["cases"].append({"case": k, "selected": picked[k], "fraction": picked[k] / n, "ms": med, "ms_all": v,
                             "ms_over_add_16": med / row["add_16_ms"], "ms_per_pixel_over_add_16": (med / picked[k]) / per_px})
    for k, v in sel.items():
        row[k + "_wall_ms"] = statistics.median(v)
        row[k + "_wall_ms_all"] = v
    print(f"{cfg} {side}^2 x {COUNT}: add_16 {row['add_16_ms']:.3f} ms (spread {100 * row['add_16_spread']:.1f} %) | " +
          " | ".join(f"{c['case']} {c['ms']:.3f} ms, {c['ms_per_pixel_over_add_16']:.2f}x per pixel" for c in row["cases"]) +
          f" | select_error {row['select_error_wall_ms']:.3f} ms, select_mask_device {row['select_mask_device_wall_ms']:.3f} ms (wall)",
          flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "adaptive_timing.json"))
    ap.add_argument("--scenes", default="C3:1024,C4:512,C5:256")
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
           "table": table}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("| config | add(16) ms | " + " | ".join(c["case"] for c in table[0]["cases"]) + " | select_error ms | select_mask_device ms |")
    for r in table:
        print(f"| {r['config']} {r['side']}^2 | {r['add_16_ms']:.2f} | " +
              " | ".join(f"{c['ms']:.2f} ({c['ms_per_pixel_over_add_16']:.2f}x)" for c in r["cases"]) +
              f" | {r['select_error_wall_ms']:.2f} | {r['select_mask_device_wall_ms']:.2f} |")


if __name__ == "__main__":
    main()
