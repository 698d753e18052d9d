"""The render kernel's wave layout, per-pixel sums and output (pix_geo, the three channel lanes, the
power-of-two reciprocal) against the oracle, exactly: ARGB ints equal and float RGB equal bit for bit.

Shapes at which that code can go wrong: a 37 x 23 frame (no multiple of any tw x th tile, so both
edges have partial tiles), spp covering every G from 1 to 64 with a partial last round and more than
one round at G = 64, one pixel per wave, row ranges with a step and bands, a refine pass, a fisheye
frame (untraced samples inside a pixel group), explicit tile lists, the calibrated dispatch order,
and each kind of variant: the ball scene runs the one with implicit primitives, the bunny the
benchmark's triangles-only one (both with the shift geometry, the channel lanes and the reciprocal),
the fisheye scene and RT_RENDER_GENERIC the all-features one (divisions, one summing lane, sums in
registers).
"""
import functools

import numpy as np
import pytest

from distraytracer_old_amd import rt, scenes
from oracle.oracle import OracleScene

pytestmark = pytest.mark.gpu

SEED = 0x5EED0001
W, H = 37, 23
BALL, FISH, BUNNY = "c3shinyBall.cli", "old_t10.cli", "c3_bun69k.cli"


@functools.lru_cache(maxsize=None)
def gpu(cli):
    return rt.Scene.load_cli(cli, textures=scenes.prepare(cli))


@functools.lru_cache(maxsize=None)
def oracle_frame(cli, spp, w=W, h=H):
    """The oracle's whole frame, computed once per (scene, spp, size) and shared read-only."""
    rgb, argb, _ = OracleScene(scenes.SCENE_DIR, cli, scenes.prepare(cli)).render(w, h, spp=spp, seed=SEED)
    rgb.setflags(write=False)
    argb.setflags(write=False)
    return rgb, argb


def assert_same(rgb, argb, ref_rgb, ref_argb, what):
    assert rgb.shape == ref_rgb.shape and argb.shape == ref_argb.shape, what
    bad = int((argb != ref_argb).sum()), int((rgb.view(np.uint32) != ref_rgb.view(np.uint32)).sum())
    dmax = float(np.abs(rgb.astype(np.float64) - ref_rgb.astype(np.float64)).max())
    print(f"{what}: argb mismatches {bad[0]}, rgb word mismatches {bad[1]}, max |d| {dmax:.3e}")
    assert bad == (0, 0), (what, bad, dmax)


@pytest.mark.parametrize("spp", [1, 2, 3, 5, 16, 17, 70, 130])
def test_every_G_and_partial_rounds(spp):
    """G = 1, 2, 2, 4, 16, 16, 64, 64: spp 3, 5, 17, 70 end in a partial round, 130 runs three rounds."""
    rgb, argb = gpu(BALL).render(W, H, spp=spp, seed=SEED)
    assert_same(rgb, argb, *oracle_frame(BALL, spp), f"spp {spp}")


@pytest.mark.parametrize("spp", [5, 16])
def test_triangles_only_variant(spp):
    """The benchmark's variant (F = 0: triangles only); the ball scene above runs the one with
    implicit primitives. Both have the shift geometry, the channel lanes and the reciprocal."""
    g = gpu(BUNNY)
    assert g.variant()[0] == 0 and gpu(BALL).variant()[0] != 0
    rgb, argb = g.render(W, H, spp=spp, seed=SEED)
    assert_same(rgb, argb, *g.render(W, H, spp=spp, seed=SEED, flags=rt.RENDER_GENERIC), f"F = 0 vs generic, spp {spp}")
    assert_same(rgb, argb, *oracle_frame(BUNNY, spp), f"F = 0 spp {spp}")


@pytest.mark.parametrize("spp", [3, 70])
def test_pixel_waves(spp):
    rgb, argb = gpu(BALL).render(W, H, spp=spp, seed=SEED, flags=rt.RENDER_PIXEL_WAVES)
    assert_same(rgb, argb, *oracle_frame(BALL, spp), f"pixel waves spp {spp}")


@pytest.mark.parametrize("band", [1, 2, 8])
def test_row_step_and_bands(band):
    """Rows 2 + k * 3 * band + j (0 <= j < band) below row 22 of the frame."""
    r0, r1, step = 2, 22, 3
    rows = [r for r in range(r0, r1) if (r - r0) % (step * band) < band]
    rgb, argb = gpu(BALL).render(W, H, spp=5, seed=SEED, rows=(r0, r1), row_step=step, row_band=band)
    ref_rgb, ref_argb = oracle_frame(BALL, 5)
    assert_same(rgb, argb, ref_rgb[rows], ref_argb[rows], f"band {band}")


def test_refine_pass_with_column_step():
    """A `refine` pass of step 4: every pixel holds the sample at the top-left of its 4 x 4 span."""
    step = 4
    rgb = np.zeros((H, W, 3), np.float32)
    argb = np.zeros((H, W), np.int32)
    gpu(BALL).render_pass(W, H, step, False, rgb, argb, spp=5, seed=SEED)
    ref_rgb, ref_argb = oracle_frame(BALL, 5)
    iy, ix = (np.arange(H) // step) * step, (np.arange(W) // step) * step
    assert_same(rgb, argb, ref_rgb[np.ix_(iy, ix)], ref_argb[np.ix_(iy, ix)], "refine step 4")


def test_fisheye_untraced_samples():
    """Pixels on the image circle have traced and untraced samples in one group of sample lanes."""
    rgb, argb = gpu(FISH).render(W, H, spp=4, seed=SEED)
    ref_rgb, ref_argb = oracle_frame(FISH, 4)
    assert (ref_argb == np.int32(-16777216)).any() and (ref_argb != np.int32(-16777216)).any()
    assert_same(rgb, argb, ref_rgb, ref_argb, "fisheye spp 4")


@pytest.mark.parametrize("spp", [3, 5])
def test_generic_variant(spp):
    """The all-features kernel: the prologue with divisions, sums in registers (G = 2, 4)."""
    rgb, argb = gpu(BALL).render(W, H, spp=spp, seed=SEED, flags=rt.RENDER_GENERIC)
    assert_same(rgb, argb, *oracle_frame(BALL, spp), f"generic spp {spp}")


def test_shuffled_tile_list():
    """Every tile of the layout through the tile-list entry, in a shuffled order, in two launches."""
    import torch

    p = rt.params(W, H, spp=5, seed=SEED)
    n, tx, tw, th = gpu(BALL).tile_layout(p)
    assert n == tx * ((H + th - 1) // th) and n > 2
    tiles = np.random.default_rng(7).permutation(n).astype(np.int32)
    rgb = torch.full((H * W, 3), -1.0, device="cuda")
    argb = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for part in (tiles[: n // 3], tiles[n // 3:]):
        gpu(BALL).render_tiles_device(p, part, rgb.data_ptr(), argb.data_ptr(), st)
    torch.cuda.synchronize()
    assert_same(rgb.cpu().numpy().reshape(H, W, 3), argb.cpu().numpy().reshape(H, W), *oracle_frame(BALL, 5), "tile list")


def test_calibrated_dispatch_order():
    """A frame large enough for the longest-first schedule (>= 2^16 pixels): the probe's order, then
    the measured one, render what the row-major dispatch renders -- the oracle's frame."""
    w, h = 261, 253
    ref = oracle_frame(BALL, 2, w, h)
    for flags in (rt.RENDER_ROWMAJOR, 0, 0, 0):
        rgb, argb = gpu(BALL).render(w, h, spp=2, seed=SEED, flags=flags)
        assert_same(rgb, argb, *ref, f"{w} x {h} flags {flags}")
