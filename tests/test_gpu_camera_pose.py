"""The camera pose on the GPU (rt_camera_rays_pose*, rt_accum_set_camera, rt_denoise_rebuild; rt.look_at). Every
comparison is byte equality unless said otherwise, against entries that were there before: Scene.camera_rays without a
pose, Scene.trace, Scene.shade, Scene.render, and the numpy restatements of the pose's arithmetic (below), of the
accumulator's fold (as tests/test_gpu_accum.py) and of the denoiser (tests/denoise_ref.py).

Two poses throughout: LOOK, a small look-at move that keeps the scenes in view, and GEN, the rotation about
(1, 2, 3) / sqrt(14) by 0.7 rad with a translation -- no symmetry, so a transposed or column-major reading of the
matrix gives other bytes.

1. Rays: camera_rays(pose=M) == xpt / xvec of camera_rays() for all five camera paths; the device entry the same.
2. Semantics: the centre ray of a look-at pose hits the sphere it looks at, at the distance geometry gives.
3. Sums: a posed accumulator's state() == its chunked state() == the fold of Scene.shade over the posed rays.
4. Adaptive: a selective add and a mixed-count add leave every pixel the fold of its own sample range.
5. set_camera: resets, equals a fresh posed accumulator, None gives the render back, the photon map is not rebuilt.
6. Denoiser: posed guides equal their definition, a run after set_camera is refused until rebuild().
7. Driver: -eye / -at writes the posed accumulator's frame; without them the output is the render's."""
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
T11_LINE, T11_SMALL = "diffuse_photons  1000000  200 0.1", "diffuse_photons  20000  50 0.1"
LOOK_EYE, LOOK_AT = (0.3, 0.2, 0.5), (0.0, 0.0, -4.0)


def _gen_pose():
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)
    m[:3, 3] = [0.8, -0.15, -0.65]  # the rotated view passes (0, 0, -2.5): every scene used here has something there
    return m


@pytest.fixture(scope="module")
def poses():
    return {"LOOK": rt.look_at(LOOK_EYE, LOOK_AT), "GEN": _gen_pose()}


@pytest.fixture(scope="module")
def scene_of(tmp_path_factory):
    """cli -> the scene, loaded once per module. "t11s.cli" is t11.cli with a small photon map, "one.cli" the
    semantics test's sphere (as tests/test_gpu_accum.py builds its own)."""
    open_scenes = {}
    d = tmp_path_factory.mktemp("pose_scenes")
    (d / "t11s.cli").write_text((scenes.SCENE_DIR / "t11.cli").read_text().replace(T11_LINE, T11_SMALL))
    (d / "one.cli").write_text("fov 60\npoint_light 0 6 0 1 1 1\nsphere 0.5 3 1 -4\n")

    def get(cli):
        if cli not in open_scenes:
            if cli in ("t11s.cli", "one.cli"):
                open_scenes[cli] = rt.Scene.load_cli(cli, scene_dir=d, textures={})
            else:
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


def _same_state(got, want, what):
    assert got[0] == want[0], (what, "samples", got[0], want[0])
    _same(got[1], want[1], (what, "sum"))
    _same(got[2], want[2], (what, "sq"))


# ---- the definition: trace_device.h's xpt / xvec over the un-posed rays ----------------------------------------
def _xform(M, p, w):
    """per row a = 0.0; a += m0 * x; a += m1 * y; a += m2 * z; a += m3 * w -- every product and sum rounded"""
    out = np.empty_like(p)
    for r in range(3):
        a = np.zeros(len(p))
        a = a + M[r, 0] * p[:, 0]
        a = a + M[r, 1] * p[:, 1]
        a = a + M[r, 2] * p[:, 2]
        a = a + M[r, 3] * w
        out[:, r] = a
    return out


def posed(rays, M):
    """the posed rays of un-posed ones; an untraced sample (d = 0) keeps d = +0"""
    M = np.asarray(M, dtype=np.float64)
    out = rays.copy()
    out["o"] = _xform(M, rays["o"], 1.0)
    out["d"] = _xform(M, rays["d"], 0.0)
    return out


def _same_rays(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    for f in ("o", "d", "tmax"):
        a = np.ascontiguousarray(got[f]).view(np.uint64).reshape(len(got), -1)
        b = np.ascontiguousarray(want[f]).view(np.uint64).reshape(len(got), -1)
        bad = np.flatnonzero((a != b).any(-1))
        assert bad.size == 0, (what, f, bad.size, bad[:8].tolist(), got[f][bad[:2]], want[f][bad[:2]])


# ---- 1. rays ---------------------------------------------------------------------------------------------------
RW, RH = 19, 17
CAMERAS = [("c3shinyBall.cli", 1), ("c3shinyBall.cli", 4), ("p2_t07.cli", 1), ("p2_t07.cli", 4), ("planets3Ortho.cli", 1),
           ("planets3Ortho.cli", 4), ("old_t10.cli", 1), ("old_t10.cli", 4)]


@pytest.mark.parametrize("cli,spp", CAMERAS)
@pytest.mark.parametrize("which", ["LOOK", "GEN"])
def test_posed_rays_are_the_transformed_rays(scene_of, poses, cli, spp, which):
    g, M = scene_of(cli), poses[which]
    for sample in range(spp):
        plain = g.camera_rays(RW, RH, spp=spp, seed=SEED, sample=sample)
        _same_rays(g.camera_rays(RW, RH, spp=spp, seed=SEED, sample=sample, pose=None), plain, (cli, spp, sample, "pose=None"))
        got = g.camera_rays(RW, RH, spp=spp, seed=SEED, sample=sample, pose=M)
        _same_rays(got, posed(plain, M), (cli, spp, sample, which))
        assert not np.array_equal(got["d"], plain["d"])  # the pose did something
        untraced = (plain["d"] == 0).all(-1)
        if cli == "old_t10.cli":  # the fisheye's corners lie outside the image circle
            assert untraced.any() and not untraced.all()
            assert not got["d"][untraced].view(np.uint64).any()  # +0, +0, +0
        else:
            assert not untraced.any()


def test_an_invalid_pose_is_refused(scene_of):
    g = scene_of("c3shinyBall.cli")
    with pytest.raises(rt.RTError, match="rt_camera_rays_pose.*orthonormal"):
        g.camera_rays(RW, RH, spp=1, pose=np.diag([2.0, 2.0, 2.0, 1.0]))
    with pytest.raises(rt.RTError, match="rt_accum_set_camera.*reflection"):
        g.accumulator(RW, RH, pose=np.diag([1.0, 1.0, -1.0, 1.0]))


@pytest.mark.parametrize("which", [None, "GEN"])
def test_rays_device_on_a_callers_stream(scene_of, poses, which):
    import torch

    from distraytracer_old_amd.desc import RAY_DTYPE

    g = scene_of("old_t10.cli")
    M = None if which is None else poses[which]
    st = torch.cuda.Stream()
    buf = torch.zeros(RW * RH * 7, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g.camera_rays_device(rt.params(RW, RH, 4, SEED), buf.data_ptr(), sample=2, stream=st.cuda_stream, pose=M)
    st.synchronize()
    got = buf.cpu().numpy().view(RAY_DTYPE).reshape(-1)
    _same_rays(got, g.camera_rays(RW, RH, spp=4, seed=SEED, sample=2, pose=M), ("device", which))


# ---- 2. semantics ----------------------------------------------------------------------------------------------
def test_the_centre_ray_hits_what_the_pose_looks_at(scene_of):
    g = scene_of("one.cli")
    eye, T = np.array([-2.0, 0.5, 1.0]), np.array([3.0, 1.0, -4.0])
    W, H = 16, 12  # even: pixel (H / 2, W / 2) is the ray through the image centre, d = (0, 0, viewZ)
    M = rt.look_at(eye, T)
    r = g.camera_rays(W, H, spp=1, seed=SEED, pose=M)
    hits = g.trace(r["o"], r["d"], seed=SEED)
    hit = ((hits["flags"] & rt.HIT_HIT) != 0).reshape(H, W)
    c = (H // 2) * W + W // 2
    assert hit[H // 2, W // 2] and hits["prim"][c] == 0
    want = np.linalg.norm(T - eye) - 0.5
    assert abs(hits["t"][c] - want) <= 1e-12 * want, (hits["t"][c], want)
    assert not hit[0, 0] and not hit[0, W - 1] and not hit[H - 1, 0] and not hit[H - 1, W - 1]
    # without the pose the sphere is not at the image centre at all
    r0 = g.camera_rays(W, H, spp=1, seed=SEED)
    assert not (g.trace(r0["o"], r0["d"], seed=SEED)["flags"][c] & rt.HIT_HIT)


# ---- 3. sums ---------------------------------------------------------------------------------------------------
CW, CH, CN = 19, 17, 16
CHUNKS = [1, 1, 2, 3, 9]
_fold_cache = {}


def _fold(g, cli, which, M, W=CW, H=CH, n=CN):
    """(n, sum, sq) [H, W, 3] of samples [0, n): sum += c and sq += c * c over the status-0 samples in sample order,
    from zeros, of Scene.shade colours over the numpy-posed Scene.camera_rays. Computed once per case, read-only."""
    key = (cli, which, W, H, n)
    if key not in _fold_cache:
        s = np.zeros((W * H, 3))
        q = np.zeros((W * H, 3))
        for k in range(n):
            r = posed(g.camera_rays(W, H, spp=max(n, 2), seed=SEED, sample=k), M)
            c, st = g.shade(r["o"], r["d"], seed=SEED, first_key=0, sample=k)
            m = st == 0
            s[m] = s[m] + c[m]
            q[m] = q[m] + c[m] * c[m]
        s.setflags(write=False)
        q.setflags(write=False)
        _fold_cache[key] = (n, s.reshape(H, W, 3), q.reshape(H, W, 3))
    return _fold_cache[key]


SUM_SCENES = ["c3shinyBall.cli", "trTrans.cli", "p2_t05.cli", "plnts3ColsBunnies.cli", "old_t10.cli", "p2_t07.cli", "t11s.cli"]


@pytest.mark.parametrize("cli", SUM_SCENES)
@pytest.mark.parametrize("which", ["LOOK", "GEN"])
def test_posed_sums_chunks_and_the_fold(scene_of, poses, cli, which):
    g, M = scene_of(cli), poses[which]
    want = _fold(g, cli, which, M)
    with g.accumulator(CW, CH, seed=SEED, moments=True, pose=M) as whole, g.accumulator(CW, CH, seed=SEED, moments=True) as cut:
        assert np.array_equal(whole.camera, M) and cut.camera is None
        cut.set_camera(M)
        whole.add(CN)
        _same_state(whole.state(), want, (cli, which, "add(16) against the fold"))
        for c in CHUNKS:
            cut.add(c)
        _same_state(cut.state(), want, (cli, which, "chunks against the fold"))
        assert len(np.unique(whole.resolve()[1])) > 1  # the frame shows something
    for flags in (rt.RENDER_GENERIC, rt.RENDER_NOCULL):
        with g.accumulator(CW, CH, seed=SEED, flags=flags, moments=True, pose=M) as b:
            b.add(CN)
            _same_state(b.state(), want, (cli, which, "flags", flags))
    with g.accumulator(CW, CH, seed=SEED, pose=M) as plain:  # the kernel without the square sums
        plain.add(CN)
        _same(plain.state()[1], want[1], (cli, which, "without moments"))


# 13 x 11 cuts every tile shape at the image edge; n = 2, 3, 5, 70: G = 2, 2, 4, 64, each but the first with a partial last round
@pytest.mark.parametrize("n", [2, 3, 5, 70])
@pytest.mark.parametrize("which", ["LOOK", "GEN"])
def test_every_wave_layout(scene_of, poses, n, which):
    cli = "c3shinyBall.cli"
    g, M = scene_of(cli), poses[which]
    want = _fold(g, cli, which, M, 13, 11, n)
    with g.accumulator(13, 11, seed=SEED, moments=True, pose=M) as a:
        a.add(n)
        _same_state(a.state(), want, (which, n))
        assert len(np.unique(a.resolve()[1])) > 1


# ---- 4. adaptive -----------------------------------------------------------------------------------------------
def _tile_checker(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return (((xs // 8) + (ys // 8)) & 1).astype(np.uint8)  # the selection's 8 x 8 tiles, every other one


@pytest.mark.parametrize("which", ["LOOK", "GEN"])
def test_selective_and_mixed_adds_fold_their_own_ranges(scene_of, poses, which):
    cli = "p2_t05.cli"
    g, M = scene_of(cli), poses[which]
    mask = _tile_checker(CW, CH).astype(bool)
    assert mask.any() and not mask.all()
    with g.accumulator(CW, CH, seed=SEED, moments=True, counts=True, pose=M) as a:
        assert a.select_mask(mask) == int(mask.sum())
        a.add_selected(3)  # samples [0, 3) of the selected pixels
        a.add(2)           # mixed counts: samples [3, 5) there, [0, 2) elsewhere
        n, s, q = a.state()
        cnt = a.counts()
    assert np.array_equal(cnt, np.where(mask, 5, 2))
    five, two = _fold(g, cli, which, M, n=5), _fold(g, cli, which, M, n=2)
    _same(s, np.where(mask[..., None], five[1], two[1]), (which, "sum"))
    _same(q, np.where(mask[..., None], five[2], two[2]), (which, "sq"))


# ---- 5. set_camera ---------------------------------------------------------------------------------------------
def test_set_camera_starts_over(scene_of, poses):
    cli = "c3shinyBall.cli"
    g = scene_of(cli)
    M1, M2 = poses["LOOK"], poses["GEN"]
    with g.accumulator(CW, CH, seed=SEED, moments=True, counts=True, pose=M1) as a, \
            g.accumulator(CW, CH, seed=SEED, moments=True, counts=True, pose=M2) as fresh:
        a.add(4)
        a.select_mask(_tile_checker(CW, CH))
        a.set_camera(M2)
        assert a.samples == 0 and np.array_equal(a.camera, M2)
        n, s, q = a.state()
        assert n == 0 and not s.view(np.uint64).any() and not q.view(np.uint64).any() and not a.counts().any()
        with pytest.raises(rt.RTError, match="rt_accum_add_selected"):
            a.add_selected(1)  # the selection went with the old camera
        a.add(4)
        fresh.add(4)
        _same_state(a.state(), fresh.state(), "set_camera(M2) + add(4) against a fresh accumulator")
        _same_state(a.state(), _fold(g, cli, "GEN", M2, n=4), "and against the fold")
        a.set_camera(None)
        assert a.camera is None and a.samples == 0
        a.add(6)
        got = a.resolve()
    rgb, argb = g.render(CW, CH, spp=6, seed=SEED)
    _same(got[0], rgb, "set_camera(None): the render again")
    assert np.array_equal(got[1], argb)


def test_the_photon_map_is_not_rebuilt(scene_of, poses):
    g = scene_of("t11s.cli")
    with g.accumulator(CW, CH, seed=SEED) as a:  # creation builds the map
        before = g.photons()
        a.set_camera(poses["LOOK"])
        a.add(2)
        a.set_camera(poses["GEN"])
        a.add(2)
        a.state()
        after = g.photons()
    assert len(before[0]) > 0
    _same(after[0], before[0], "photon positions")
    _same(after[1], before[1], "photon powers")


# ---- 6. denoiser -----------------------------------------------------------------------------------------------
def _guides_of(g, W, H, M):
    """the header's guide definition over the posed centre rays"""
    r = posed(g.camera_rays(W, H, spp=1, seed=SEED, sample=0), M)
    hits = g.trace(r["o"], r["d"], seed=SEED, first_key=0)
    hit = (hits["flags"] & rt.HIT_HIT) != 0
    e = hits["pos"] - r["o"]
    depth = np.sqrt(((e[:, 0] * e[:, 0]) + (e[:, 1] * e[:, 1])) + (e[:, 2] * e[:, 2])).astype(np.float32)
    zero = np.float32(0)
    assert hit.any() and not hit.all()
    return {"normal": np.where(hit[:, None], hits["normal"].astype(np.float32), zero).reshape(H, W, 3),
            "pos": np.where(hit[:, None], hits["pos"].astype(np.float32), zero).reshape(H, W, 3),
            "depth": np.where(hit, depth, zero).reshape(H, W),
            "material": np.where(hit, hits["material"], -1).astype(np.int32).reshape(H, W)}


def test_denoiser_follows_the_camera(scene_of, poses):
    cli, W, H = "old_t10.cli", 20, 18  # fisheye: rejected centre rays among the guides
    g = scene_of(cli)
    M1, M2 = poses["LOOK"], poses["GEN"]
    with g.accumulator(W, H, seed=SEED, moments=True, pose=M1) as a, a.denoiser() as d:
        got = d.guides()
        want = _guides_of(g, W, H, M1)
        for k in want:
            _same(got[k], want[k], (cli, "LOOK", k))
        a.add(4)
        d.run(levels=1)
        a.set_camera(M2)
        a.add(4)
        for run in (lambda: d.run(levels=1), lambda: d.run_device(0, 0, levels=1)):
            with pytest.raises(rt.RTError, match="rt_denoise_run.*another camera"):
                run()
        d.rebuild()
        with pytest.raises(rt.RTError, match="rt_denoise_planes"):
            d.planes()  # the planes were of the old guides
        got = d.guides()
        with a.denoiser() as fresh:
            made = fresh.guides()
        want = _guides_of(g, W, H, M2)
        for k in want:
            _same(got[k], made[k], (cli, "rebuild against a fresh denoiser", k))
            _same(got[k], want[k], (cli, "GEN", k))
        d.rebuild()  # again: into the same buffers
        for k in want:
            _same(d.guides()[k], want[k], (cli, "second rebuild", k))
        p = rt.DenoiseParams.defaults()
        rgb, argb = d.run(levels=3)
        _, s, q = a.state()
        c, v = ref.run(s, q, np.full((H, W), 4), want, 3, p.normal_log2, p.sigma_l, p.sigma_z)
        pc, pv = d.planes()
        _same(pc, c, "colour plane")
        _same(pv, v, "variance plane")
        want_rgb, want_argb = ref.output(c)
        _same(rgb, want_rgb, "rgb")
        assert np.array_equal(argb, want_argb)


# ---- 7. driver -------------------------------------------------------------------------------------------------
def test_driver_eye_and_at(scene_of, tmp_path):
    from PIL import Image

    native.build()
    exe = tmp_path / "rtrender"
    subprocess.run(["g++", "-O2", "-std=c++17", str(REPO / "tools" / "rtrender.cpp"), "-o", str(exe), f"-L{native.LIB_DIR}",
                    "-ldistraytracer", "-lz", f"-Wl,-rpath,{native.LIB_DIR}"], check=True, capture_output=True)
    W, H = 48, 40
    cli = "c3shinyBall.cli"
    g = scene_of(cli)
    base = [str(exe), str(scenes.SCENE_DIR), cli, "-w", str(W), "-h", str(H), "-seed", str(SEED), "-spp", "4"]
    eye, at, up = (1.5, 1.0, 1.0), (0.0, 0.5, -3.0), (0.1, 1.0, 0.0)
    out = tmp_path / "posed.png"
    r = subprocess.run(base + ["-o", str(out), "-eye", *map(str, eye), "-at", *map(str, at), "-up", *map(str, up)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with g.accumulator(W, H, seed=SEED, pose=rt.look_at(eye, at, up)) as a:
        a.add(4)
        _, argb = a.resolve()
    img = np.asarray(Image.open(out).convert("RGB")).astype(np.uint8)
    assert np.array_equal(img, rt.argb_to_rgb8(argb))
    assert len(np.unique(argb)) > 1
    plain = tmp_path / "plain.png"
    r = subprocess.run(base + ["-o", str(plain)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, argb0 = g.render(W, H, spp=4, seed=SEED)
    img0 = np.asarray(Image.open(plain).convert("RGB")).astype(np.uint8)
    assert np.array_equal(img0, rt.argb_to_rgb8(argb0)) and not np.array_equal(img0, img)
    r = subprocess.run(base + ["-o", str(plain), "-eye", "0", "0", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "-at" in r.stderr  # -eye without -at
