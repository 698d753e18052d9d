"""Radiance queries on the GPU: rt_shade_rays runs the render kernel's shading tree on caller rays, and
rt_camera_rays hands out the rays a frame shoots. Every comparison is byte equality.

1. A frame from queries equals the frame: the camera rays of every sample, shaded under the frame's keys
   and folded on the host in fp64 as render_kernel folds them, give rt_render's rgb and argb bit for bit,
   on fifteen scenes that each cover one thing (see FRAMES).
2. Independent camera: rays built in numpy (tests/trace_util.camera_rays) give the same frame, and equal
   Scene.camera_rays byte for byte.
3. Invariances on rays that are no camera rays: one ray per call with its own key, RT_TRACE_SORT,
   RT_TRACE_GENERIC, RT_TRACE_NOCULL, the device entry, small staging chunks; a miss returns the background.
4. Edges: batch sizes around the wave size, rejected rays at the wave's ends and as a whole wave, status=None."""
import ctypes

import numpy as np
import pytest

from distraytracer_old_amd import desc, rt, scenes
from tests import trace_util as tu

pytestmark = pytest.mark.gpu

SEED = 0x5EED0001
T11_LINE, T11_SMALL = "diffuse_photons  1000000  200 0.1", "diffuse_photons  20000  50 0.1"


# ---- the host fold (render_kernel's epilogue) ---------------------------------------------------------
def _jd2i(x):
    """Java's (int) of a double: NaN -> 0, saturating, towards zero."""
    x = np.where(np.isnan(x), 0.0, x)
    return np.trunc(np.clip(x, -2147483648.0, 2147483647.0)).astype(np.int64)


def _pack(c):
    """myColor.getInt of fp64 colours [n, 3] -> int32 [n], with uint32 wrap-around as the kernel adds."""
    q = _jd2i(c * 255) & 0xFFFFFFFF
    v = ((255 << 24) + ((q[:, 0] << 16) & 0xFFFFFFFF) + ((q[:, 1] << 8) & 0xFFFFFFFF) + q[:, 2]) & 0xFFFFFFFF
    return v.astype(np.uint32).view(np.int32)


def _fold(cols, stats, spp, dof):
    """Per-sample colours [spp][n, 3] and status bytes [spp][n] -> the pixels' fp64 colours [n, 3]: at 1 spp
    without DOF the colour as returned; else the sum from +0.0 over the traced samples in sample order,
    divided by spp, clamped to <= 1 (clampc)."""
    if spp == 1 and not dof:
        return cols[0]
    acc = np.zeros_like(cols[0])
    for c, s in zip(cols, stats):
        m = s == 0
        acc[m] = acc[m] + c[m]
    return np.minimum(1.0, acc / float(spp))


def _has_lens(text):
    return any(line.split()[:1] == ["lens"] for line in text.splitlines())


def _frame_from_queries(g, W, H, spp, dof, rays_of=None, **kw):
    """(rgb float32 [H, W, 3], argb int32 [H, W], status bytes [spp][n]) of the frame folded from queries."""
    cols, stats = [], []
    for s in range(spp):
        r = rays_of(s) if rays_of else g.camera_rays(W, H, spp=spp, seed=SEED, sample=s)
        c, st = g.shade(r["o"], r["d"], seed=SEED, first_key=0, sample=s, **kw)
        cols.append(c)
        stats.append(st)
    c = _fold(cols, stats, spp, dof)
    return c.astype(np.float32).reshape(H, W, 3), _pack(c).reshape(H, W), stats


def _assert_frame(got_rgb, got_argb, rgb, argb, what):
    bad = np.flatnonzero((got_rgb.view(np.uint32) != rgb.view(np.uint32)).any(-1).ravel())
    assert bad.size == 0, (what, "rgb", bad.size, bad[:8].tolist())
    assert np.array_equal(got_argb, argb), (what, "argb", int((got_argb != argb).sum()))


# ---- 1. a frame from queries equals the frame --------------------------------------------------------
# (scene, W, H, spp): what it covers
FRAMES = [
    ("c3shinyBall.cli", 64, 48, 1),      # reflection frames, width != height
    ("c3_bun69k.cli", 64, 64, 4),        # jitter order, BVH
    ("c2clear.cli", 64, 64, 1),
    ("trTrans.cli", 64, 64, 2),          # both Fresnel children
    ("p2_t05.cli", 64, 64, 2),           # disk light: shadow RNG sites keyed by pixel, sample and node
    ("c3spotLight.cli", 64, 64, 2),      # spot light
    ("p2_t03.cli", 64, 64, 2),           # moving sphere's time draw
    ("p2_t07.cli", 64, 64, 2),           # DOF, non-zero origins
    ("old_t10.cli", 64, 64, 1),          # fisheye, untraced samples: status 2, colour 0
    ("old_t10.cli", 64, 64, 4),          # ... skipped by the fold
    ("planets3Ortho.cli", 64, 64, 2),    # ortho
    ("p4_t05.cli", 64, 64, 1),
    ("p3_t09.cli", 64, 64, 2),           # procedural noise: fails if the unit's Perlin tables were not uploaded
    ("plnts3ColsBunnies.cli", 48, 48, 2),  # C4's mask, image textures, instances
    ("p3_t11_sierp.cli", 64, 64, 1),
]


@pytest.mark.parametrize("cli,W,H,spp", FRAMES)
def test_frame_from_queries_equals_the_frame(cli, W, H, spp):
    scenes.ensure_bun69k()
    dof = _has_lens((scenes.SCENE_DIR / cli).read_text())
    assert dof == (cli == "p2_t07.cli")
    with rt.Scene.load_cli(cli, textures=scenes.prepare(cli)) as g:
        rgb, argb = g.render(W, H, spp=spp, seed=SEED)
        got_rgb, got_argb, stats = _frame_from_queries(g, W, H, spp, dof)
        _assert_frame(got_rgb, got_argb, rgb, argb, (cli, W, H, spp))
        rejected = sum(int((s == 2).sum()) for s in stats)
        if cli == "old_t10.cli":  # the corners lie outside the image circle
            assert rejected > 0 and all(set(np.unique(s)) <= {0, 2} for s in stats)
            r = g.camera_rays(W, H, spp=spp, seed=SEED, sample=0)
            out = stats[0] == 2
            assert not r["d"][out].any() and r["d"][~out].any(1).all()
        else:
            assert rejected == 0
        assert np.isinf(g.camera_rays(W, H, spp=spp, seed=SEED, sample=spp - 1)["tmax"]).all()
        assert len(np.unique(argb)) > 1  # the frame shows something


@pytest.fixture(scope="module")
def t11_small(tmp_path_factory):
    """t11.cli with a small photon map (as test_gpu_parity.py), and that map's photon_list, built once."""
    d = tmp_path_factory.mktemp("shade_t11")
    (d / "t11s.cli").write_text((scenes.SCENE_DIR / "t11.cli").read_text().replace(T11_LINE, T11_SMALL))
    with rt.Scene.load_cli("t11s.cli", scene_dir=d, textures={}) as b:
        b.build_photons(SEED)
        pos, pwr = b.photons()
    assert len(pos) > 1000
    return d, pos, pwr


def test_frame_from_queries_photon_map(t11_small):
    """t11 (C5's mask, the photon gather): the same photon_list set on the rendering and on the queried scene."""
    d, pos, pwr = t11_small
    W = H = 64
    with rt.Scene.load_cli("t11s.cli", scene_dir=d, textures={}) as a, rt.Scene.load_cli("t11s.cli", scene_dir=d, textures={}) as b:
        a.set_photons(pos, pwr)
        b.set_photons(pos, pwr)
        rgb, argb = a.render(W, H, spp=1, seed=SEED)
        got_rgb, got_argb, _ = _frame_from_queries(b, W, H, 1, False)
        _assert_frame(got_rgb, got_argb, rgb, argb, "t11s")
        assert len(np.unique(argb)) > 1


def test_photon_map_is_built_on_demand_with_the_calls_seed(t11_small):
    """A shade call on a scene that uses a photon map builds it with p->seed, as a render does."""
    d, _, _ = t11_small
    W = H = 32
    o, dd = tu.camera_rays(W, H, 60.0)
    with rt.Scene.load_cli("t11s.cli", scene_dir=d, textures={}) as a, rt.Scene.load_cli("t11s.cli", scene_dir=d, textures={}) as b:
        assert a.info()["photons"] == 0
        c, st = a.shade(o, dd, seed=SEED, first_key=0, sample=0)
        assert a.info()["photons"] > 1000 and not st.any()
        rgb, argb = b.render(W, H, spp=1, seed=SEED)  # builds its map with the same seed
        _assert_frame(c.astype(np.float32).reshape(H, W, 3), _pack(c).reshape(H, W), rgb, argb, "on demand")


# ---- 2. independent camera ----------------------------------------------------------------------------
@pytest.mark.parametrize("cli,W,H", [("t01.cli", 64, 64), ("c3shinyBall.cli", 64, 48)])
def test_numpy_camera_rays_give_the_frame(cli, W, H):
    o, d = tu.camera_rays(W, H, 60.0)
    mine = rt.rays(o, d)
    with rt.Scene.load_cli(cli, textures=scenes.prepare(cli)) as g:
        theirs = g.camera_rays(W, H, spp=1, seed=SEED, sample=0)
        assert theirs.dtype == desc.RAY_DTYPE and theirs.tobytes() == mine.tobytes()
        rgb, argb = g.render(W, H, spp=1, seed=SEED)
        got_rgb, got_argb, _ = _frame_from_queries(g, W, H, 1, False, rays_of=lambda s: mine)
        _assert_frame(got_rgb, got_argb, rgb, argb, cli)
        # the device entry writes the same rays
        import torch

        dev = torch.device("cuda", 0)
        t = torch.zeros(W * H * desc.RAY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        g.camera_rays_device(rt.params(W, H, 1, SEED), t.data_ptr(), sample=0)
        torch.cuda.synchronize(dev)
        assert t.cpu().numpy().tobytes() == mine.tobytes()
        # the sample index is checked against spp, the layout must be the whole frame
        for bad in (dict(sample=1), dict(sample=-1)):
            with pytest.raises(rt.RTError, match="rt_camera_rays: sample"):
                g.camera_rays(W, H, spp=1, seed=SEED, **bad)
        p = rt.params(W, H, 1, SEED, rows=(0, H // 2))
        assert rt.lib().rt_camera_rays(g._h, ctypes.byref(p), 0, theirs.ctypes.data) == -1


# ---- 3. invariances on non-camera rays ---------------------------------------------------------------
KEY = dict(seed=77, first_key=1000, sample=3)
N = 4099


@pytest.fixture(scope="module")
def gen_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("shade_scenes")
    (d / "gen_b.cli").write_text(tu.scene_text("b"))
    return d


@pytest.fixture(scope="module")
def gen_b(gen_dir):
    """The generated scene b (ground, BVH, a transparent sphere), its 4099 incoherent rays and their colours."""
    g = rt.Scene.load_cli("gen_b.cli", scene_dir=gen_dir, textures={})
    o, d = tu.incoherent_rays(tu.bvh_world_tris("b"), N)
    rgb, st = g.shade(o, d, **KEY)
    assert not st.any() and len(np.unique(rgb, axis=0)) > 16
    yield g, o, d, rgb, st
    g.close()


def _hemisphere_rays(g, W, seed):
    """Bounce rays off the scene's camera hits: a random direction in the hemisphere of each hit's normal."""
    o, d = tu.camera_rays(W, W, 60.0)
    h = g.trace(o, d)
    h = h[(h["flags"] & rt.HIT_HIT) != 0]
    v = np.random.default_rng(seed).normal(size=(len(h), 3))
    v *= np.where((v * h["normal"]).sum(1, keepdims=True) < 0, -1.0, 1.0)
    return h["pos"] + 1e-4 * h["normal"], v


@pytest.fixture(scope="module")
def bunny():
    scenes.ensure_bun69k()
    g = rt.Scene.load_cli("c3_bun69k.cli", textures=scenes.prepare("c3_bun69k.cli"))
    o, d = _hemisphere_rays(g, 64, 5)
    assert len(o) > 500
    rgb, st = g.shade(o, d, **KEY)
    assert not st.any()
    yield g, o, d, rgb, st
    g.close()


def _same(got, want, what):
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes(), (what, np.flatnonzero((a != b).reshape(len(a), -1).any(1))[:8].tolist())


@pytest.mark.parametrize("which", ["gen_b", "bunny"])
def test_a_ray_alone_with_its_own_key_gets_the_same_colour(which, request):
    """A shuffled batch, position by position: each ray traced in a call of its own under its own key."""
    g, o, d, rgb, st = request.getfixturevalue(which)
    perm = np.random.default_rng(9).permutation(len(o))[:192]
    for i in perm:
        c, s = g.shade(o[i:i + 1], d[i:i + 1], seed=KEY["seed"], first_key=KEY["first_key"] + int(i), sample=KEY["sample"])
        assert c.tobytes() == rgb[i:i + 1].tobytes() and s[0] == 0, int(i)
    # and a slice of the batch under its first ray's key
    a, b = 1000 % len(o), min(len(o), 1000 % len(o) + 130)
    _same(g.shade(o[a:b], d[a:b], seed=KEY["seed"], first_key=KEY["first_key"] + a, sample=KEY["sample"]), (rgb[a:b], st[a:b]), "slice")


def test_the_key_matters_where_the_scene_draws_random_numbers():
    """p2_t05's disk light draws its shadow points from the ray's key: the colour follows the key (pixel and
    sample), not the ray's place in the batch."""
    cli, W = "p2_t05.cli", 32
    with rt.Scene.load_cli(cli, textures=scenes.prepare(cli)) as g:
        r = g.camera_rays(W, W, spp=2, seed=SEED, sample=1)
        o, d = r["o"], r["d"]
        base, _ = g.shade(o, d, seed=SEED, first_key=0, sample=1)
        assert g.shade(o, d, seed=SEED, first_key=5, sample=1)[0].tobytes() != base.tobytes()
        assert g.shade(o, d, seed=SEED, first_key=0, sample=0)[0].tobytes() != base.tobytes()
        assert g.shade(o, d, seed=SEED + 1, first_key=0, sample=1)[0].tobytes() != base.tobytes()
        perm = np.random.default_rng(2).permutation(W * W)
        for i in perm[:128]:
            c, _ = g.shade(o[i:i + 1], d[i:i + 1], seed=SEED, first_key=int(i), sample=1)
            assert c.tobytes() == base[i:i + 1].tobytes(), int(i)
        for fl in (rt.TRACE_SORT, rt.TRACE_GENERIC, rt.TRACE_NOCULL):
            assert g.shade(o[perm], d[perm], seed=SEED, first_key=0, sample=1, flags=fl)[0].tobytes() == \
                g.shade(o[perm], d[perm], seed=SEED, first_key=0, sample=1)[0].tobytes(), fl


@pytest.mark.parametrize("which", ["gen_b", "bunny"])
@pytest.mark.parametrize("flag", ["SORT", "GENERIC", "NOCULL", "SORT|GENERIC|NOCULL"])
def test_flags_return_the_same_bytes(which, flag, request):
    g, o, d, rgb, st = request.getfixturevalue(which)
    fl = 0
    for f in flag.split("|"):
        fl |= getattr(rt, "TRACE_" + f)
    _same(g.shade(o, d, flags=fl, **KEY), (rgb, st), flag)


@pytest.mark.parametrize("which", ["gen_b", "bunny"])
def test_device_entry_returns_the_same_bytes(which, request):
    import torch

    g, o, d, rgb, st = request.getfixturevalue(which)
    r = rt.rays(o, d)
    n = len(r)
    dev = torch.device("cuda", 0)
    t_rays = torch.from_numpy(r.view(np.uint8).reshape(-1)).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    for fl in (0, rt.TRACE_SORT):
        with torch.cuda.stream(side):
            t_rgb = torch.full((n, 3), 7.0, dtype=torch.float64, device=dev)
            t_st = torch.full((n,), 7, dtype=torch.uint8, device=dev)
            g.shade_device(t_rays.data_ptr(), n, t_rgb.data_ptr(), t_st.data_ptr(), stream=side.cuda_stream, flags=fl, **KEY)
            t_rgb2 = torch.full((n, 3), 7.0, dtype=torch.float64, device=dev)
            g.shade_device(t_rays.data_ptr(), n, t_rgb2.data_ptr(), 0, stream=side.cuda_stream, flags=fl, **KEY)
        side.synchronize()
        _same((t_rgb.cpu().numpy(), t_st.cpu().numpy()), (rgb, st), ("device", fl))
        assert t_rgb2.cpu().numpy().tobytes() == rgb.tobytes()


def test_small_staging_chunks_return_the_same_bytes(gen_b, gen_dir, monkeypatch):
    g, o, d, rgb, st = gen_b
    monkeypatch.setenv("DISTRAYTRACER_TRACE_CHUNK", "1000")
    with rt.Scene.load_cli("gen_b.cli", scene_dir=gen_dir, textures={}) as h:
        assert len(o) == 4099
        _same(h.shade(o, d, **KEY), (rgb, st), "chunks")
        _same(h.shade(o, d, flags=rt.TRACE_SORT, **KEY), (rgb, st), "sorted chunks")
        W = 48  # 2304 camera rays through three chunks
        assert h.camera_rays(W, W, spp=1, seed=SEED).tobytes() == g.camera_rays(W, W, spp=1, seed=SEED).tobytes()


def test_a_miss_returns_the_background(gen_b):
    g, o, d, rgb, st = gen_b
    miss = (g.trace(o, d, seed=KEY["seed"], first_key=KEY["first_key"])["flags"] & rt.HIT_HIT) == 0
    assert 16 < miss.sum() < len(o)
    bg = np.array([0.1, 0.1, 0.2])  # scene_text's `background 0.1 0.1 0.2`, no skydome
    assert rgb[miss].tobytes() == np.tile(bg, (int(miss.sum()), 1)).tobytes()


# ---- 4. edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_batch_sizes_around_the_wave_size(n, gen_b):
    g, o, d, rgb, st = gen_b
    for fl in (0, rt.TRACE_SORT):
        c, s = g.shade(o[:n], d[:n], flags=fl, **KEY)
        assert c.shape == (n, 3) and c.dtype == np.float64 and s.shape == (n,) and s.dtype == np.uint8
        _same((c, s), (rgb[:n], st[:n]), (n, fl))


def _spoil(o, d, idx):
    """Make the rays idx rejected ones, cycling through NaN origin, +-Inf direction, zero direction, NaN direction."""
    for j, i in enumerate(idx):
        k = j % 4
        if k == 0:
            o[i, j % 3] = np.nan
        elif k == 1:
            d[i, j % 3] = np.inf if j % 8 < 4 else -np.inf
        elif k == 2:
            d[i] = [0.0, -0.0, 0.0]
        else:
            d[i, (j + 1) % 3] = np.nan


def _assert_rejected(g, o, d, rgb, idx, what):
    o, d = o.copy(), d.copy()
    _spoil(o, d, idx)
    want_rgb, want_st = rgb[:len(o)].copy(), np.zeros(len(o), np.uint8)
    want_rgb[idx] = 0.0
    want_st[idx] = 2
    for fl in (0, rt.TRACE_SORT):
        c, s = g.shade(o, d, flags=fl, **KEY)
        _same((c, s), (want_rgb, want_st), (what, fl))
        c2, s2 = g.shade(o, d, flags=fl, status=None, **KEY)
        assert s2 is None and c2.tobytes() == want_rgb.tobytes(), (what, fl, "status=None")


def test_a_wave_of_rejected_rays_between_two_good_waves(gen_b):
    g, o, d, rgb, st = gen_b
    _assert_rejected(g, o[:192], d[:192], rgb, list(range(64, 128)), "wave")


def test_rejected_rays_at_lane_0_lane_63_and_the_tail(gen_b):
    g, o, d, rgb, st = gen_b
    _assert_rejected(g, o, d, rgb, [0, 63, 64, 127, 2048, 4032, 4095, 4096, 4098], "lanes")
    _assert_rejected(g, o[:65], d[:65], rgb, [64], "tail lane")
    _assert_rejected(g, o[:64], d[:64], rgb, list(range(64)), "all rejected")
