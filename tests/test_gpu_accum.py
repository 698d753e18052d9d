"""Progressive sample accumulation on the GPU (rt_accum_*, rt.Accumulator). Every comparison is byte equality.
The yardsticks are entries that were there before: Scene.render for frames, and Scene.camera_rays plus
Scene.shade folded in numpy for the raw sums.

1. Resolve equals the render: add(n), resolve() == Scene.render(spp=n), over scenes that each cover one
   thing and sizes that cut every tile shape at the image edge, with every sample-lane count G.
2. Chunk invariance and the sums themselves: state() after add(16) == state() after the chunks 1, 1, 2, 3, 9
   == the numpy fold of the shaded camera rays.
3. Progressive: after each of those chunks resolve() == render(spp=done) wherever done >= 2.
4. Checkpoint: state() / restore() into a fresh accumulator, reset(), two accumulators on one scene.
5. RENDER_GENERIC / RENDER_NOCULL give the same bytes; resolve_device on a caller's stream == resolve().
6. The error map equals its definition evaluated in numpy from state().
7. The driver's -budget mode writes the frame of the samples it reports."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from distraytracer_old_amd import build as native
from distraytracer_old_amd import rt, scenes

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
SEED = 0x5EED0001
T11_LINE, T11_SMALL = "diffuse_photons  1000000  200 0.1", "diffuse_photons  20000  50 0.1"


@pytest.fixture(scope="module")
def scene_of(tmp_path_factory):
    """cli -> the scene, loaded once per module. "t11s.cli" is t11.cli with a small photon map (as
    test_gpu_parity.py), built on demand by whichever entry needs it first."""
    open_scenes = {}
    d = tmp_path_factory.mktemp("accum_t11")
    (d / "t11s.cli").write_text((scenes.SCENE_DIR / "t11.cli").read_text().replace(T11_LINE, T11_SMALL))

    def get(cli):
        if cli not in open_scenes:
            if cli == "t11s.cli":
                open_scenes[cli] = rt.Scene.load_cli(cli, scene_dir=d, textures={})
            else:
                scenes.ensure_bun69k()
                open_scenes[cli] = rt.Scene.load_cli(cli, textures=scenes.prepare(cli))
        return open_scenes[cli]

    yield get
    for g in open_scenes.values():
        g.close()


def _same_frame(got, want, what):
    (got_rgb, got_argb), (rgb, argb) = got, want
    assert got_rgb.shape == rgb.shape and got_argb.shape == argb.shape, what
    bad = np.flatnonzero((got_rgb.view(np.uint32) != rgb.view(np.uint32)).any(-1).ravel())
    assert bad.size == 0, (what, "rgb", bad.size, bad[:8].tolist())
    assert np.array_equal(got_argb, argb), (what, "argb", int((got_argb != argb).sum()))


def _same_state(got, want, what):
    assert got[0] == want[0], (what, "samples", got[0], want[0])
    for name, a, b in (("sum", got[1], want[1]), ("sq", got[2], want[2])):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).any(-1).ravel())
            assert bad.size == 0, (what, name, bad.size, bad[:8].tolist())


# ---- 1. resolve equals the render ---------------------------------------------------------------------
# (scene, W, H, n). G = the largest power of two <= min(n, 64); the tiles are 8x8 (G = 1), 8x4, 4x4, 4x2,
# 2x2, 2x1, 1x1 (G = 64): 13 x 11 cuts all of them at the right and bottom edge.
RESOLVE = [("c3shinyBall.cli", 13, 11, n) for n in (2, 3, 4, 5, 8, 16, 32, 64, 70)] + [  # n = 3, 5, 70: a partial last round
    ("c3_bun69k.cli", 64, 64, 4),          # the BVH, mask 0
    ("trTrans.cli", 32, 32, 2),            # both Fresnel children
    ("p2_t05.cli", 32, 32, 2),             # disk light: shadow RNG sites keyed by pixel, sample and node
    ("p2_t03.cli", 32, 32, 2),             # moving sphere's time draw
    ("p3_t09.cli", 32, 32, 2),             # procedural noise: this unit's Perlin tables
    ("plnts3ColsBunnies.cli", 24, 24, 2),  # C4's mask, image textures, instances
    ("planets3Ortho.cli", 32, 32, 3),      # ortho
    ("old_t10.cli", 32, 32, 4),            # fisheye: untraced samples are skipped but counted
    ("p2_t07.cli", 32, 32, 1),             # DOF: a 1-spp render shoots the lens ray too
    ("p2_t07.cli", 32, 32, 3),
    ("t11s.cli", 32, 32, 2),               # C5's mask: the photon map built on demand by rt_accum_create
]


@pytest.mark.parametrize("cli,W,H,n", RESOLVE)
def test_resolve_equals_the_render(scene_of, cli, W, H, n):
    g = scene_of(cli)
    with g.accumulator(W, H, seed=SEED) as a:
        assert a.samples == 0
        a.add(n)
        assert a.samples == n
        got = a.resolve()
    want = g.render(W, H, spp=n, seed=SEED)
    _same_frame(got, want, (cli, W, H, n))
    assert len(np.unique(want[1])) > 1  # the frame shows something


# ---- 2, 3. chunk invariance, the sums themselves, progressive frames ------------------------------------
CW, CH, CN = 19, 17, 16
CHUNKS = [1, 1, 2, 3, 9]
_fold_cache = {}


def _fold(g, cli):
    """(16, sum, sq) [CH, CW, 3] of the first 16 samples: sum += c and sq += c * c over the status-0 samples in
    sample order, from zeros, of Scene.shade colours over Scene.camera_rays. Computed once per scene."""
    if cli not in _fold_cache:
        s = np.zeros((CW * CH, 3))
        q = np.zeros((CW * CH, 3))
        untraced = 0
        for k in range(CN):
            r = g.camera_rays(CW, CH, spp=CN, seed=SEED, sample=k)
            c, st = g.shade(r["o"], r["d"], seed=SEED, first_key=0, sample=k)
            m = st == 0
            untraced += int((~m).sum())
            s[m] = s[m] + c[m]
            q[m] = q[m] + c[m] * c[m]
        s.setflags(write=False)
        q.setflags(write=False)
        _fold_cache[cli] = ((CN, s.reshape(CH, CW, 3), q.reshape(CH, CW, 3)), untraced)
    return _fold_cache[cli]


@pytest.mark.parametrize("cli", ["p2_t05.cli", "old_t10.cli"])
def test_chunks_sums_and_progressive_frames(scene_of, cli):
    g = scene_of(cli)
    want, untraced = _fold(g, cli)
    assert (untraced > 0) == (cli == "old_t10.cli")  # the fisheye's corners lie outside the image circle
    with g.accumulator(CW, CH, seed=SEED, moments=True) as whole, g.accumulator(CW, CH, seed=SEED, moments=True) as cut:
        whole.add(CN)
        _same_state(whole.state(), want, (cli, "add(16) against the fold"))
        for c in CHUNKS:
            cut.add(c)
            done = cut.samples
            if done >= 2:  # 2, 4, 7, 16
                _same_frame(cut.resolve(), g.render(CW, CH, spp=done, seed=SEED), (cli, "progressive", done))
        assert cut.samples == CN
        _same_state(cut.state(), want, (cli, "chunks against the fold"))
        _same_state(cut.state(), whole.state(), (cli, "chunks against add(16)"))
    assert want[1].any() and want[2].any()


# ---- 4. checkpoint ---------------------------------------------------------------------------------------
def test_checkpoint_reset_and_two_accumulators(scene_of):
    cli = "p2_t05.cli"
    g = scene_of(cli)
    want, _ = _fold(g, cli)
    with g.accumulator(CW, CH, seed=SEED, moments=True) as a:
        a.add(5)
        n, s, q = a.state()
        assert n == 5
    with g.accumulator(CW, CH, seed=SEED, moments=True) as b:
        b.restore(n, s, q)
        assert b.samples == 5
        b.add(11)
        _same_state(b.state(), want, "restore(5) + add(11)")
        b.reset()
        assert b.samples == 0
        z = b.state()
        assert not z[1].view(np.uint64).any() and not z[2].view(np.uint64).any()  # +0.0 everywhere
        with pytest.raises(rt.RTError, match="rt_accum_resolve"):
            b.resolve()
        b.add(CN)
        _same_state(b.state(), want, "reset() + add(16)")
    with g.accumulator(CW, CH, seed=SEED, moments=True) as x, g.accumulator(CW, CH, seed=SEED) as y:
        x.add(3)
        y.add(CN)
        x.add(13)
        _same_state(x.state(), want, "interleaved, with moments")
        _same_state(y.state(), (want[0], want[1], None), "interleaved, without moments")
        with pytest.raises(rt.RTError, match="rt_accum_restore"):
            y.restore(n, s, q)  # sq given to an accumulator without moments
        with pytest.raises(rt.RTError, match="rt_accum_restore"):
            x.restore(n, s)  # sq missing
        with pytest.raises(rt.RTError, match="rt_accum_error"):
            y.error()


# ---- 5. flags and device entries -----------------------------------------------------------------------------
@pytest.mark.parametrize("cli", ["p2_t05.cli", "c3shinyBall.cli"])
@pytest.mark.parametrize("flags", [rt.RENDER_GENERIC, rt.RENDER_NOCULL, rt.RENDER_GENERIC | rt.RENDER_NOCULL])
def test_generic_and_nocull_give_the_same_bytes(scene_of, cli, flags):
    g = scene_of(cli)
    with g.accumulator(CW, CH, seed=SEED, moments=True) as a, g.accumulator(CW, CH, seed=SEED, flags=flags, moments=True) as b:
        a.add(6)
        b.add(6)
        _same_state(b.state(), a.state(), (cli, flags))


def test_refused_render_flags(scene_of):
    g = scene_of("c3shinyBall.cli")
    for flags in (rt.RENDER_SHCOMPACT, rt.RENDER_WAVEFRONT, rt.RENDER_PIXEL_WAVES):
        with pytest.raises(rt.RTError, match="rt_accum_create"):
            g.accumulator(CW, CH, flags=flags)


def test_device_entries_on_a_callers_stream(scene_of):
    import torch

    g = scene_of("p2_t05.cli")
    st = torch.cuda.Stream()
    rgb = torch.zeros((CH, CW, 3), dtype=torch.float32, device="cuda")
    argb = torch.zeros((CH, CW), dtype=torch.int32, device="cuda")
    err = torch.zeros((CH, CW), dtype=torch.float32, device="cuda")
    only = torch.zeros((CH, CW), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with g.accumulator(CW, CH, seed=SEED, moments=True) as a:
        a.add(3, stream=st.cuda_stream)  # the add, the resolve and the error map ordered by the stream
        a.add(4, stream=st.cuda_stream)
        a.resolve_device(rgb.data_ptr(), argb.data_ptr(), stream=st.cuda_stream)
        a.resolve_device(0, only.data_ptr(), stream=st.cuda_stream)  # either output may be null
        a.error_device(err.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        want = a.resolve()  # synchronises the stream of the last add itself
        want_err = a.error()
    _same_frame((rgb.cpu().numpy(), argb.cpu().numpy()), want, "resolve_device")
    assert np.array_equal(only.cpu().numpy(), want[1])
    assert np.array_equal(err.cpu().numpy().view(np.uint32), want_err.view(np.uint32))
    _same_frame(want, g.render(CW, CH, spp=7, seed=SEED), "resolve after adds on a caller's stream")


# ---- 6. error map --------------------------------------------------------------------------------------------
def test_error_map_equals_its_definition(scene_of):
    g = scene_of("p2_t05.cli")
    with g.accumulator(CW, CH, seed=SEED, moments=True) as a:
        a.add(1)
        with pytest.raises(rt.RTError, match="rt_accum_error"):
            a.error()  # n < 2
        a.add(CN - 1)
        got = a.error()
        n, s, q = a.state()
    assert n == CN
    m = s / n
    v = q / n - m * m
    v = np.where(v < 0, 0.0, v)
    e = np.sqrt((v * n / (n - 1)) / n)
    want = e.max(-1).astype(np.float32)
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (bad.size, bad[:8].tolist(), got.ravel()[bad[:4]], want.ravel()[bad[:4]])
    assert got.max() > 0 and np.isfinite(got).all()


# ---- 7. driver -----------------------------------------------------------------------------------------------
def test_driver_budget(scene_of, tmp_path):
    from PIL import Image

    native.build()
    exe = tmp_path / "rtrender"
    subprocess.run(["g++", "-O2", "-std=c++17", str(REPO / "tools" / "rtrender.cpp"), "-o", str(exe), f"-L{native.LIB_DIR}",
                    "-ldistraytracer", "-lz", f"-Wl,-rpath,{native.LIB_DIR}"], check=True, capture_output=True)
    out = tmp_path / "b.png"
    W, H = 48, 40
    r = subprocess.run([str(exe), str(scenes.SCENE_DIR), "c3shinyBall.cli", "-w", str(W), "-h", str(H), "-seed", str(SEED),
                        "-budget", "30", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("samples ")]
    assert len(lines) == 1 and len(lines[0]) == 2, r.stdout
    n = int(lines[0][1])
    assert n >= 2
    _, argb = scene_of("c3shinyBall.cli").render(W, H, spp=n, seed=SEED)
    img = np.asarray(Image.open(out).convert("RGB")).astype(np.uint8)
    assert np.array_equal(img, rt.argb_to_rgb8(argb)), n
