"""How much closer to the converged frame the denoiser brings a low-sample frame, and which sigma_z does it best.

Per case (scene, size, samples n): the mean squared error of the raw resolve and of the denoised frame against
Scene.render(spp=1024) with the same seed, over the float rgb; the denoised frame for every sigma_z of the sweep, the
other parameters at their defaults. The ratio denoised / raw below 1 is a gain.

    python tools/denoise_quality.py [--out FILE] [--cases p2_t05.cli:64:4,p3_t09.cli:64:16,c3_bun69k.cli:64:4]
        writes profiles/denoise_quality.json and prints the table of DESIGN.md section 17.
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

from distraytracer_old_amd import rt, scenes  # noqa: E402

SEED = 0x5EED0001
TRUTH_SPP = 1024
SIGMA_Z = (0.001, 0.003, 0.01, 0.03, 0.1, 0.3, 1.0)


def measure(cli, side, n):
    with rt.Scene.load_cli(cli, textures=scenes.prepare(cli)) as g:
        truth = g.render(side, side, spp=TRUTH_SPP, seed=SEED)[0].astype(np.float64)
        with g.accumulator(side, side, seed=SEED, moments=True) as a, a.denoiser() as d:
            a.add(n)
            raw = a.resolve()[0].astype(np.float64)
            mse_raw = float(((raw - truth) ** 2).mean())
            sweep = []
            for sz in SIGMA_Z:
                den = d.run(sigma_z=sz)[0].astype(np.float64)
                mse = float(((den - truth) ** 2).mean())
                sweep.append({"sigma_z": sz, "mse": mse, "ratio": mse / mse_raw})
            den = d.run()[0].astype(np.float64)
            mse_def = float(((den - truth) ** 2).mean())
    row = {"scene": cli, "side": side, "samples": n, "truth_spp": TRUTH_SPP, "mse_raw": mse_raw, "mse_denoised_defaults": mse_def,
           "ratio_defaults": mse_def / mse_raw, "sigma_z_sweep": sweep}
    print(f"{cli} {side}^2 n={n}: raw {mse_raw:.4e} | defaults {mse_def:.4e} ratio {row['ratio_defaults']:.4f} | " +
          " ".join(f"{s['sigma_z']}:{s['ratio']:.4f}" for s in sweep), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "denoise_quality.json"))
    ap.add_argument("--cases", default="p2_t05.cli:64:4,p3_t09.cli:64:16,c3_bun69k.cli:64:4")
    a = ap.parse_args()
    scenes.ensure_bun69k()
    d = rt.DenoiseParams.defaults()
    table = [measure(c.split(":")[0], int(c.split(":")[1]), int(c.split(":")[2])) for c in a.cases.split(",")]
    out = {"build_id": rt.build_id(), "seed": SEED,
           "defaults": {"levels": d.levels, "normal_log2": d.normal_log2, "sigma_l": d.sigma_l, "sigma_z": d.sigma_z}, "table": table}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
