"""The variance-guided a-trous denoiser on the GPU (rt_denoise_*, rt.Denoiser). Every comparison is byte equality
unless said otherwise. The yardsticks are entries that were there before -- Scene.camera_rays plus Scene.trace for the
guides, Accumulator.resolve / state / counts and Scene.render for frames -- and the filter's restatement in numpy
(tests/denoise_ref.py), which tests/test_denoise_ref.py checks on its own.

Sizes: 13 x 11 (one partial block; from stride 16 on every tap but the centre is outside), 40 x 36 (nine row tiles of
one partial segment), 70 x 9 (two segments per row, the second 6 pixels wide; a last tile of one row)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from distraytracer_old_amd import build as native
from distraytracer_old_amd import rt, scenes
from tests import denoise_ref as ref

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
SEED = 0x5EED0001


@pytest.fixture(scope="module")
def scene_of():
    open_scenes = {}

    def get(cli):
        if cli not in open_scenes:
            scenes.ensure_bun69k()
            open_scenes[cli] = rt.Scene.load_cli(cli, textures=scenes.prepare(cli))
        return open_scenes[cli]

    yield get
    for g in open_scenes.values():
        g.close()


def _same(x, y, what):
    assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape, x.dtype, y.dtype)
    w = {8: np.uint64, 4: np.uint32}[x.dtype.itemsize]
    bad = np.flatnonzero(np.ascontiguousarray(x).view(w).ravel() != np.ascontiguousarray(y).view(w).ravel())
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def _defaults(**over):
    p = rt.DenoiseParams.defaults(**over)
    return dict(normal_log2=p.normal_log2, sigma_l=p.sigma_l, sigma_z=p.sigma_z)


def _check_levels(a, d, n, levels, what, **over):
    """planes() and the frame after each of `levels` equal the restatement, computed level by level"""
    _, s, q = a.state()
    g = d.guides()
    par = _defaults(**over)
    c, v = ref.init(s, q, n)
    done = 0
    for L in sorted(levels):
        for i in range(done, L):
            c, v = ref.level(c, v, n, g, 1 << i, **par)
        done = L
        rgb, argb = d.run(levels=L, **over)
        pc, pv = d.planes()
        _same(pc, c, (what, L, "colour plane"))
        _same(pv, v, (what, L, "variance plane"))
        want_rgb, want_argb = ref.output(c)
        _same(rgb, want_rgb, (what, L, "rgb"))
        assert np.array_equal(argb, want_argb), (what, L, "argb")
    return c, v


# ---- guides ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cli,W,H", [("c3shinyBall.cli", 13, 11), ("old_t10.cli", 32, 32), ("plnts3ColsBunnies.cli", 24, 24),
                                     ("p2_t03.cli", 32, 32)])
def test_guides_are_the_traced_centre_rays(scene_of, cli, W, H):
    g = scene_of(cli)
    r = g.camera_rays(W, H, spp=1, seed=SEED, sample=0)
    hits = g.trace(r["o"], r["d"], seed=SEED, first_key=0)
    hit = (hits["flags"] & rt.HIT_HIT) != 0
    e = hits["pos"] - r["o"]
    depth = np.sqrt(((e[:, 0] * e[:, 0]) + (e[:, 1] * e[:, 1])) + (e[:, 2] * e[:, 2])).astype(np.float32)
    zero = np.float32(0)
    want = {"normal": np.where(hit[:, None], hits["normal"].astype(np.float32), zero).reshape(H, W, 3),
            "pos": np.where(hit[:, None], hits["pos"].astype(np.float32), zero).reshape(H, W, 3),
            "depth": np.where(hit, depth, zero).reshape(H, W),
            "material": np.where(hit, hits["material"], -1).astype(np.int32).reshape(H, W)}
    with g.accumulator(W, H, seed=SEED, moments=True) as a, a.denoiser() as d:
        got = d.guides()
    for k in want:
        _same(got[k], want[k], (cli, k))
    assert hit.any()
    if cli == "old_t10.cli":  # the fisheye's corners: rejected rays
        assert (r["d"] == 0).all(-1).any() and (got["material"] == -1).any()
        assert (got["depth"][got["material"] == -1] == 0).all()


def test_create_needs_moments_and_run_needs_samples(scene_of):
    g = scene_of("c3shinyBall.cli")
    with g.accumulator(8, 8, seed=SEED) as a:
        with pytest.raises(rt.RTError, match="rt_denoise_create"):
            a.denoiser()
    for counts in (False, True):
        with g.accumulator(8, 8, seed=SEED, moments=True, counts=counts) as a, a.denoiser() as d:
            with pytest.raises(rt.RTError, match="rt_denoise_run"):
                d.run()
            with pytest.raises(rt.RTError, match="rt_denoise_planes"):
                d.planes()


# ---- levels = 0 is resolve -----------------------------------------------------------------------------------
def _checker(H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    return ((xs // 3 + ys // 2) & 1).astype(np.uint8)


def test_zero_levels_is_resolve(scene_of):
    g = scene_of("c3shinyBall.cli")
    W, H = 13, 11
    with g.accumulator(W, H, seed=SEED, moments=True, counts=True) as a, a.denoiser() as d:
        a.add(3)
        rgb, argb = d.run(levels=0)
        want_rgb, want_argb = a.resolve()
        _same(rgb, want_rgb, "uniform counts")
        assert np.array_equal(argb, want_argb)
        a.select_mask(_checker(H, W))
        a.add_selected(2)
        rgb, argb = d.run(levels=0)
        want_rgb, want_argb = a.resolve()
        _same(rgb, want_rgb, "mixed counts")
        assert np.array_equal(argb, want_argb)
    with g.accumulator(W, H, seed=SEED, moments=True) as a, a.denoiser() as d:  # one sample: v = 1 everywhere
        a.add(1)
        rgb, argb = d.run(levels=0)
        _same(rgb, a.resolve()[0], "one sample")
        assert (d.planes()[1] == 1.0).all()


# ---- the planes against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("cli,W,H", [("c3shinyBall.cli", 13, 11), ("p2_t05.cli", 40, 36), ("c3shinyBall.cli", 70, 9)])
def test_planes_equal_the_restatement(scene_of, cli, W, H):
    g = scene_of(cli)
    with g.accumulator(W, H, seed=SEED, moments=True) as a, a.denoiser() as d:
        a.add(4)
        n = np.full((H, W), 4)
        c5, _ = _check_levels(a, d, n, [1, 2, 3, 4, 5], (cli, W, H))
        c0, _ = ref.init(*a.state()[1:], n)
        assert not np.array_equal(c5, c0)  # the filter did something
        if (W, H) == (13, 11):  # strides 32, 64, 128 leave the centre tap alone
            _check_levels(a, d, n, [8], (cli, W, H))


# ---- mixed counts ----------------------------------------------------------------------------------------------
def test_mixed_counts(scene_of):
    cli, W, H = "p2_t05.cli", 40, 36
    g = scene_of(cli)
    with g.accumulator(W, H, seed=SEED, moments=True, counts=True) as a, a.denoiser() as d:
        a.add(2)
        a.select_mask(_checker(H, W))
        a.add_selected(3)
        n = a.counts()
        assert sorted(np.unique(n).tolist()) == [2, 5]
        _check_levels(a, d, n, [1, 3], "add(2), add_selected(3) on a checkerboard")
        # a checkpoint with pixels of no and of one sample among the counts
        _, s, q = a.state()
        n2 = n.copy()
        n2[3:6, 4:9] = 0
        n2[0, 0] = n2[H - 1, W - 1] = n2[20, 17] = 0
        n2[10:12, 30:40] = 1
        a.restore(5, s, q)
        a.restore_counts(n2)
        c, v = _check_levels(a, d, n2, [0, 1, 4], "restored counts with zeros and ones")
        rgb, argb = d.run(levels=4)
        assert (rgb[n2 == 0] == 0).all() and (argb[n2 == 0].view(np.uint32) == 0xFF000000).all()
        assert (c[n2 == 0] == 0).all() and (v[n2 == 0] == 1.0).all()
        d.run(levels=0)
        assert (d.planes()[1][n2 == 1] == 1.0).all()


# ---- parameters --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [dict(normal_log2=0), dict(normal_log2=10), dict(sigma_l=1.0), dict(sigma_l=16.0),
                                  dict(sigma_z=0.001), dict(sigma_z=1.0)], ids=lambda o: "%s=%s" % next(iter(o.items())))
def test_parameters(scene_of, over):
    cli, W, H = "plnts3ColsBunnies.cli", 24, 24
    g = scene_of(cli)
    with g.accumulator(W, H, seed=SEED, moments=True) as a, a.denoiser() as d:
        a.add(4)
        _check_levels(a, d, np.full((H, W), 4), [2], (cli, over), **over)


# ---- a caller's stream -------------------------------------------------------------------------------------------
def test_run_device_on_a_callers_stream(scene_of):
    import torch

    cli, W, H = "c3shinyBall.cli", 70, 9
    g = scene_of(cli)
    dev = torch.device("cuda:0")
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    argb = torch.zeros((H, W), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    with g.accumulator(W, H, seed=SEED, moments=True) as a, a.denoiser() as d:
        a.add(4, stream=st.cuda_stream)
        d.run_device(rgb.data_ptr(), argb.data_ptr(), stream=st.cuda_stream, levels=3)
        st.synchronize()
        pc, pv = d.planes()
        want_rgb, want_argb = d.run(levels=3)
        _same(rgb.cpu().numpy(), want_rgb, "run_device rgb")
        assert np.array_equal(argb.cpu().numpy(), want_argb)
        c, v = d.planes()
        _same(pc, c, "planes of the device run")
        _same(pv, v, "variance of the device run")


# ---- a run disturbs nothing ------------------------------------------------------------------------------------------
def test_a_run_leaves_the_accumulator_alone(scene_of):
    cli, W, H = "c3shinyBall.cli", 13, 11
    g = scene_of(cli)
    with g.accumulator(W, H, seed=SEED, moments=True, counts=True) as a, a.denoiser() as d:
        a.add(3)
        before = a.state(), a.counts()
        d.run()
        after = a.state(), a.counts()
        assert before[0][0] == after[0][0] == 3
        _same(before[0][1], after[0][1], "sum")
        _same(before[0][2], after[0][2], "sq")
        assert np.array_equal(before[1], after[1])
        a.add(2)
        rgb, argb = a.resolve()
        want_rgb, want_argb = g.render(W, H, spp=5, seed=SEED)
        _same(rgb, want_rgb, "add after a run")
        assert np.array_equal(argb, want_argb)
        a.select_mask(_checker(H, W))
        a.add_selected(2)
        cnt = a.counts()
        d.run()
        assert np.array_equal(a.counts(), cnt)
        want7 = g.render(W, H, spp=7, seed=SEED)[0]
        got = a.resolve()[0]
        _same(got[cnt == 7], want7[cnt == 7], "selected pixels after a run")
        _same(got[cnt == 5], want_rgb[cnt == 5], "the others")


# ---- quality -----------------------------------------------------------------------------------------------------
def test_denoised_soft_shadows_are_closer_to_the_converged_frame(scene_of, capsys):
    cli, W, H, n = "p2_t05.cli", 64, 64, 4
    g = scene_of(cli)
    truth = g.render(W, H, spp=1024, seed=SEED)[0].astype(np.float64)
    with g.accumulator(W, H, seed=SEED, moments=True) as a, a.denoiser() as d:
        a.add(n)
        raw = a.resolve()[0].astype(np.float64)
        den = d.run()[0].astype(np.float64)
    mse_raw, mse_den = float(((raw - truth) ** 2).mean()), float(((den - truth) ** 2).mean())
    with capsys.disabled():
        print(f"\n{cli} {W}x{H} n={n}: mse raw {mse_raw:.6e} denoised {mse_den:.6e} ratio {mse_den / mse_raw:.4f}")
    assert mse_den < mse_raw


# ---- driver --------------------------------------------------------------------------------------------------------
def test_driver_denoise(scene_of, tmp_path):
    from PIL import Image

    cli, W, H = "c3shinyBall.cli", 32, 32
    native.build()
    exe = tmp_path / "rtrender"
    subprocess.run(["g++", "-O2", "-std=c++17", str(REPO / "tools" / "rtrender.cpp"), "-o", str(exe), f"-L{native.LIB_DIR}",
                    "-ldistraytracer", "-lz", f"-Wl,-rpath,{native.LIB_DIR}"], check=True, capture_output=True)
    out, f32 = tmp_path / "d.png", tmp_path / "d.f32"
    r = subprocess.run([str(exe), str(scenes.SCENE_DIR), cli, "-w", str(W), "-h", str(H), "-seed", str(SEED), "-spp", "4",
                        "-denoise", "-o", str(out), "-rgb", str(f32)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = scene_of(cli)
    with g.accumulator(W, H, seed=SEED, moments=True) as a, a.denoiser() as d:
        a.add(4)
        rgb, argb = d.run()
        raw = a.resolve()[1]
    assert not np.array_equal(argb, raw)
    img = np.asarray(Image.open(out).convert("RGB")).astype(np.uint8)
    assert np.array_equal(img, rt.argb_to_rgb8(argb))
    _same(np.fromfile(f32, dtype=np.float32).reshape(H, W, 3), rgb, "-rgb")
    # -spp 1 cannot be denoised; an explicit level count is taken
    r = subprocess.run([str(exe), str(scenes.SCENE_DIR), cli, "-w", "8", "-h", "8", "-spp", "1", "-denoise", "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "-denoise" in r.stderr
