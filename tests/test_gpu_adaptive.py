"""Adaptive sampling on the GPU (RT_ACCUM_COUNTS, rt_accum_select_*, rt_accum_add_selected). Every comparison is
byte equality. The yardsticks are entries that were there before: Scene.render for frames, Scene.camera_rays plus
Scene.shade folded in numpy for the raw sums, and an accumulator without counts for whole-frame adds.

1. A pixel with n samples holds Scene.render(spp=n) at that pixel: three masks in turn with chunks 1, 3 and 8
   (list lengths that are no multiple of the wave's 64 / G entries), then one mask with a chunk of every G.
2. The same on the feature scenes (BVH, transparency, disk light, textures, fisheye, lens, photon map).
3. The raw sums equal the numpy fold of the shaded camera rays, taken to each pixel's own count.
4. Chunk invariance; an all-pixels selection equals add(), also as a procedural-noise scene's first shading;
   RENDER_GENERIC / RENDER_NOCULL give the same bytes.
5. The selection is the mask's pixels in the documented tile-major order, from a host or a device mask.
6. select_error selects the numpy predicate's pixels; the error map of per-pixel counts equals its definition.
7. Checkpoint with counts; reset. 8. A caller's stream. 9. The driver's -noise mode."""
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
    """cli -> the scene, loaded once per module ("t11s.cli": t11.cli with a small photon map, as test_gpu_accum.py)."""
    open_scenes = {}
    d = tmp_path_factory.mktemp("adaptive_t11")
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


_renders = {}


def _render(g, cli, W, H, n):
    """Scene.render(spp=n), computed once per (scene, size, n) and left unchanged"""
    key = (cli, W, H, n)
    if key not in _renders:
        rgb, argb = g.render(W, H, spp=n, seed=SEED)
        rgb.setflags(write=False)
        argb.setflags(write=False)
        _renders[key] = (rgb, argb)
    return _renders[key]


def _frame_is_the_render_per_count(g, cli, a, W, H, what):
    """every pixel of a's frame equals render(spp = its count) there; -> the distinct counts"""
    cnt = a.counts()
    rgb, argb = a.resolve()
    for n in np.unique(cnt).tolist():
        assert n >= 2, (what, n)
        want_rgb, want_argb = _render(g, cli, W, H, n)
        at = cnt == n
        bad = np.flatnonzero(((rgb.view(np.uint32) != want_rgb.view(np.uint32)).any(-1) & at).ravel())
        assert bad.size == 0, (what, "rgb", n, bad.size, bad[:8].tolist())
        assert np.array_equal(argb[at], want_argb[at]), (what, "argb", n)
    return np.unique(cnt).tolist()


def _same(x, y, what):
    assert x.shape == y.shape and x.dtype == y.dtype, what
    w = {8: np.uint64, 4: np.uint32}[x.dtype.itemsize]
    bad = np.flatnonzero(x.view(w).ravel() != y.view(w).ravel())
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def _same_all(a, b, what):
    """sum, sq and cnt of two accumulators"""
    (na, sa, qa), (nb, sb, qb) = a.state(), b.state()
    assert na == nb, (what, "samples")
    _same(sa, sb, (what, "sum"))
    if qa is not None or qb is not None:
        _same(qa, qb, (what, "sq"))
    _same(a.counts(), b.counts(), (what, "cnt"))


def _checker(W, H):
    r, c = np.mgrid[0:H, 0:W]
    return (r + c) % 2 == 0


# ---- 1. per-pixel equality with the render -------------------------------------------------------------------
BW, BH = 13, 11


def _ball_masks():
    m1 = _checker(BW, BH)  # 72 pixels, pixel 0 and the last one among them
    m2 = np.zeros((BH, BW), dtype=bool)
    m2[4, 5] = True  # one lone pixel
    m2[:, -1] = True  # and the last column: 12 pixels
    m3 = np.ones((BH, BW), dtype=bool)  # 143
    return m1, m2, m3


def test_every_pixel_is_the_render_of_its_own_count(scene_of):
    cli = "c3shinyBall.cli"
    g = scene_of(cli)
    masks = _ball_masks()
    assert masks[0][0, 0] and masks[0][-1, -1]
    # entries per wave 64 / G: c = 1 -> 64, c = 3 -> 32, c = 8 -> 8; none divides its list's length
    for m, c in zip(masks, (1, 3, 8)):
        G = 1 << (min(c, 64).bit_length() - 1)
        assert int(m.sum()) % (64 // G) != 0
    with g.accumulator(BW, BH, seed=SEED, moments=True, counts=True) as a:
        a.add(2)
        for m, c in zip(masks, (1, 3, 8)):
            assert a.select_mask(m) == int(m.sum())
            a.add_selected(c)
        assert a.samples == 2  # what add() gave every pixel
        want = 2 + masks[0] * 1 + masks[1] * 3 + masks[2] * 8
        assert np.array_equal(a.counts(), want)
        distinct = _frame_is_the_render_per_count(g, cli, a, BW, BH, "three masks")
    assert len(distinct) >= 4, distinct


@pytest.mark.parametrize("c", [2, 4, 5, 16, 64, 70])  # G = 2, 4, 4, 16, 64, 64; 5 and 70 end in a partial round
def test_every_sample_lane_count(scene_of, c):
    cli = "c3shinyBall.cli"
    g = scene_of(cli)
    m = _ball_masks()[1] | (_checker(BW, BH) & (np.arange(BW) < 7))  # 12 + a left-hand checkerboard
    with g.accumulator(BW, BH, seed=SEED, moments=True, counts=True) as a:
        a.add(2)
        a.select_mask(m)
        a.add_selected(c)
        assert np.array_equal(a.counts(), 2 + m * c)
        _frame_is_the_render_per_count(g, cli, a, BW, BH, ("G", c))


# ---- 2. the feature scenes ---------------------------------------------------------------------------------------
FEATURES = [("c3_bun69k.cli", 64, 64),          # the packet BVH, with wave-mates that are not neighbours
            ("trTrans.cli", 32, 32),            # both Fresnel children
            ("p2_t05.cli", 32, 32),             # disk light: shadow RNG sites keyed by pixel, sample and node
            ("plnts3ColsBunnies.cli", 24, 24),  # C4's mask, image textures, instances
            ("old_t10.cli", 32, 32),            # fisheye: untraced samples are skipped but counted
            ("p2_t07.cli", 32, 32),             # the lens
            ("t11s.cli", 32, 32)]               # C5's mask: the photon map


@pytest.mark.parametrize("cli,W,H", FEATURES)
def test_feature_scenes(scene_of, cli, W, H):
    g = scene_of(cli)
    m = _checker(W, H)  # half the frame, no two selected pixels side by side
    with g.accumulator(W, H, seed=SEED, counts=True) as a:
        a.add(2)
        assert a.select_mask(m) == W * H // 2
        a.add_selected(3)
        assert _frame_is_the_render_per_count(g, cli, a, W, H, cli) == [2, 5]
    assert len(np.unique(_render(g, cli, W, H, 5)[1])) > 1  # the frame shows something


# ---- 3. raw sums ---------------------------------------------------------------------------------------------
CW, CH = 19, 17


def _seq_masks():
    r, c = np.mgrid[0:CH, 0:CW]
    return (r + 2 * c) % 3 == 0, c >= r  # overlapping: counts 2, 5, 7 and 10


def _masked_sequence(a):
    mA, mB = _seq_masks()
    a.add(2)
    a.select_mask(mA)
    a.add_selected(3)
    a.select_mask(mB)
    a.add_selected(5)
    return 2 + mA * 3 + mB * 5


@pytest.mark.parametrize("cli", ["p2_t05.cli", "old_t10.cli"])
def test_raw_sums_are_the_fold_to_each_pixels_count(scene_of, cli):
    g = scene_of(cli)
    with g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as a:
        want_cnt = _masked_sequence(a)
        cnt = a.counts()
        _, got_s, got_q = a.state()
    assert np.array_equal(cnt, want_cnt) and sorted(np.unique(cnt).tolist()) == [2, 5, 7, 10]
    s = np.zeros((CW * CH, 3))
    q = np.zeros((CW * CH, 3))
    untraced = 0
    for k in range(int(cnt.max())):
        r = g.camera_rays(CW, CH, spp=16, seed=SEED, sample=k)
        col, st = g.shade(r["o"], r["d"], seed=SEED, first_key=0, sample=k)
        untraced += int((st != 0).sum())
        m = (st == 0) & (k < cnt.ravel())
        s[m] = s[m] + col[m]
        q[m] = q[m] + col[m] * col[m]
    assert (untraced > 0) == (cli == "old_t10.cli")
    _same(got_s, s.reshape(CH, CW, 3), (cli, "sum"))
    _same(got_q, q.reshape(CH, CW, 3), (cli, "sq"))
    assert s.any() and q.any()


# ---- 4. invariance -------------------------------------------------------------------------------------------
def test_chunk_invariance_and_all_pixels(scene_of):
    g = scene_of("p2_t05.cli")
    mA, _ = _seq_masks()
    every = np.ones((CH, CW), dtype=bool)
    with g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as a, \
            g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as b:
        for x in (a, b):
            x.add(2)
            x.select_mask(mA)
        a.add_selected(3)
        a.add_selected(5)
        b.add_selected(8)
        _same_all(a, b, "3 + 5 against 8")
        # add() once the counts are mixed: samples [cnt[p], cnt[p] + 3) of every pixel, as an all-pixels selection
        a.add(3)
        b.select_mask(every)
        b.add_selected(3)
        assert a.samples == 5 and b.samples == 2
        _same(a.counts(), b.counts(), "add against an all-pixels selection, cnt")
        _same(a.state()[1], b.state()[1], "add against an all-pixels selection, sum")
        _same(a.state()[2], b.state()[2], "add against an all-pixels selection, sq")
    for n in (1, 6, 16):
        with g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as a, g.accumulator(CW, CH, seed=SEED, moments=True) as b:
            assert a.select_mask(every) == CW * CH
            a.add_selected(n)
            b.add(n)
            assert (a.counts() == n).all() and a.samples == 0 and b.samples == n
            _same(a.state()[1], b.state()[1], ("all pixels against add", n, "sum"))
            _same(a.state()[2], b.state()[2], ("all pixels against add", n, "sq"))


def test_procedural_noise_on_a_scene_that_has_not_rendered(scene_of):
    """The selective add's kernels read their own translation unit's copy of the Perlin tables. On a scene with
    procedural wood whose first shading is add_selected, an all-pixels selection equals the plain accumulator's add."""
    cli, W, H, n = "p3_t09.cli", 32, 32, 2
    g = scene_of(cli)  # no other test of this module opens it
    every = np.ones((H, W), dtype=bool)
    with g.accumulator(W, H, seed=SEED, moments=True, counts=True) as a, g.accumulator(W, H, seed=SEED, moments=True) as b:
        assert a.select_mask(every) == W * H
        a.add_selected(n)
        b.add(n)
        assert (a.counts() == n).all()
        _same(a.state()[1], b.state()[1], (cli, "sum"))
        _same(a.state()[2], b.state()[2], (cli, "sq"))
        assert len(np.unique(a.state()[1])) > 16  # the frame shows something


@pytest.mark.parametrize("cli", ["p2_t05.cli", "c3shinyBall.cli"])
@pytest.mark.parametrize("flags", [rt.RENDER_GENERIC, rt.RENDER_NOCULL])
def test_generic_and_nocull_give_the_same_bytes(scene_of, cli, flags):
    g = scene_of(cli)
    with g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as a, \
            g.accumulator(CW, CH, seed=SEED, flags=flags, moments=True, counts=True) as b:
        _masked_sequence(a)
        _masked_sequence(b)
        _same_all(a, b, (cli, flags))


# ---- 5. selection --------------------------------------------------------------------------------------------
def _tile_major(W, H):
    """every pixel index of a W x H image in the selection's order: 8 x 8 tiles row-major, Morton inside"""
    out = []
    for ty in range((H + 7) // 8):
        for tx in range((W + 7) // 8):
            for code in range(64):
                dx = (code & 1) | ((code >> 1) & 2) | ((code >> 2) & 4)
                dy = ((code >> 1) & 1) | ((code >> 2) & 2) | ((code >> 3) & 4)
                col, row = tx * 8 + dx, ty * 8 + dy
                if col < W and row < H:
                    out.append(row * W + col)
    return np.array(out, dtype=np.int32)


# Past 256 tiles select_scan_kernel's 256 threads take ceil(ntiles / 256) counts each: 2056 x 8 and 8 x 2056 are 257
# tiles (two a thread, thread 128 half-filled, threads 129.. empty), 136 x 136 is 289. The masks in the loop below are a
# random one, the full one and a checkerboard, each followed by the empty one.
@pytest.mark.parametrize("W,H", [(13, 11), (70, 9), (2056, 8), (8, 2056), (136, 136)])
def test_selection_is_the_mask_in_tile_major_order(scene_of, W, H):
    import torch

    g = scene_of("c3shinyBall.cli")
    order = _tile_major(W, H)
    assert sorted(order.tolist()) == list(range(W * H)) and order[:4].tolist() == [0, 1, W, W + 1]
    rng = np.random.default_rng(7)
    with g.accumulator(W, H, seed=SEED, counts=True) as a:
        with pytest.raises(rt.RTError, match="rt_accum_selection"):
            a.selection()
        for m in (rng.random((H, W)) < 0.4, np.ones((H, W), dtype=bool), _checker(W, H)):
            want = order[m.ravel()[order]]
            assert a.select_mask(m) == want.size
            assert np.array_equal(a.selection(), want)
            d = torch.from_numpy(m.astype(np.uint8)).cuda()
            assert a.select_mask(np.zeros((H, W), dtype=bool)) == 0 and a.selection().size == 0
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            assert a.select_mask_device(d.data_ptr(), stream=st.cuda_stream) == want.size
            assert np.array_equal(a.selection(), want)


def test_an_empty_selection_adds_nothing(scene_of):
    g = scene_of("p2_t05.cli")
    with g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as a:
        with pytest.raises(rt.RTError, match="rt_accum_add_selected"):
            a.add_selected(1)  # no selection yet
        a.add(3)
        before = a.state(), a.counts()
        assert a.select_mask(np.zeros((CH, CW), dtype=bool)) == 0
        a.add_selected(4)
        after = a.state(), a.counts()
        assert before[0][0] == after[0][0] == 3
        _same(after[0][1], before[0][1], "sum")
        _same(after[0][2], before[0][2], "sq")
        _same(after[1], before[1], "cnt")
        assert (after[1] == 3).all()


# ---- 6. error selection ----------------------------------------------------------------------------------------
def _error_of(s, q, cnt):
    """rt_accum_error's definition with n = cnt per pixel; +Inf below two samples"""
    n = cnt.astype(np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = s / n
        v = q / n - m * m
        v = np.where(v < 0, 0.0, v)
        e = np.sqrt((v * n / (n - 1)) / n).max(-1).astype(np.float32)
    return np.where(cnt < 2, np.float32(np.inf), e)


def test_select_error(scene_of):
    g = scene_of("p2_t05.cli")
    W = H = 32
    order = _tile_major(W, H)
    with g.accumulator(W, H, seed=SEED, moments=True, counts=True) as a:
        a.add(8)
        _, s, q = a.state()
        e = _error_of(s, q, a.counts())
        _same(a.error(), e, "error map, uniform counts")
        thr = np.float32(0.5) * e[np.isfinite(e)].max()
        assert thr.dtype == np.float32 and thr > 0

        def predicate(e, cnt, top):
            return (cnt < top) & ((cnt < 2) | ~(e <= thr))

        want = order[predicate(e, a.counts(), 1024).ravel()[order]]
        assert 0 < want.size < W * H
        assert a.select_error(float(thr), 1024) == want.size
        assert np.array_equal(a.selection(), want)
        assert a.select_error(float(thr), 8) == 0  # every pixel has its 8 samples
        assert a.select_error(float(thr), 9) == want.size
        a.add_selected(3)
        cnt = a.counts()
        assert sorted(np.unique(cnt).tolist()) == [8, 11]
        _, s, q = a.state()
        e = _error_of(s, q, cnt)
        _same(a.error(), e, "error map, per-pixel counts")
        want = order[predicate(e, cnt, 11).ravel()[order]]  # the pixels at 11 are out, whatever their error
        assert a.select_error(float(thr), 11) == want.size
        assert np.array_equal(a.selection(), want)
        assert (cnt.ravel()[want] == 8).all()


def test_fewer_than_two_samples(scene_of):
    g = scene_of("p2_t05.cli")
    half = _checker(CW, CH)
    with g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as a:
        assert a.select_error(0.0, 4) == CW * CH  # no samples at all
        with pytest.raises(rt.RTError, match="rt_accum_error"):
            a.error()  # no add of any kind yet
        with pytest.raises(rt.RTError, match="rt_accum_resolve"):
            a.resolve()
        a.add(1)
        assert np.isposinf(a.error()).all()
        assert a.select_error(1e30, 4) == CW * CH  # one sample: selected whatever the threshold
        assert a.select_error(1e30, 1) == 0
        a.select_mask(half)
        a.add_selected(1)
        cnt = a.counts()
        assert np.array_equal(cnt, 1 + half)
        _, s, q = a.state()
        got = a.error()
        _same(got, _error_of(s, q, cnt), "error map with +Inf")
        assert np.isposinf(got[~half]).all() and np.isfinite(got[half]).all()
    with g.accumulator(CW, CH, seed=SEED, counts=True) as b:  # a pixel without samples resolves black
        b.select_mask(half)
        b.add_selected(2)
        rgb, argb = b.resolve()
        assert not rgb[~half].view(np.uint32).any() and (argb[~half].view(np.uint32) == 0xFF000000).all()
        want_rgb, want_argb = g.render(CW, CH, spp=2, seed=SEED)
        _same(rgb[half], want_rgb[half], "rgb")
        assert np.array_equal(argb[half], want_argb[half])
        with pytest.raises(rt.RTError, match="rt_accum_select_error"):
            b.select_error(0.1, 4)  # no moments


# ---- 7. checkpoint -------------------------------------------------------------------------------------------
def test_checkpoint_with_counts_and_reset(scene_of):
    g = scene_of("p2_t05.cli")
    mA, mB = _seq_masks()
    with g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as a, \
            g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as b:
        _masked_sequence(a)
        n, s, q = a.state()
        cnt = a.counts()
        assert n == 2
        b.restore(n, s, q)
        assert (b.counts() == 2).all()  # restore alone: every pixel at `samples`
        b.restore_counts(cnt)
        _same_all(a, b, "restored")
        with pytest.raises(rt.RTError, match="rt_accum_add_selected"):
            b.add_selected(1)  # the selection did not survive the restore
        for x in (a, b):
            x.select_mask(mA ^ mB)
            x.add_selected(4)
        _same_all(a, b, "one more chunk on both")
        with pytest.raises(rt.RTError, match="rt_accum_restore_counts"):
            b.restore_counts(np.full((CH, CW), -1, dtype=np.int32))
        b.reset()
        assert b.samples == 0 and not b.counts().any()
        z = b.state()
        assert not z[1].view(np.uint64).any() and not z[2].view(np.uint64).any()
        with pytest.raises(rt.RTError, match="rt_accum_add_selected"):
            b.add_selected(1)  # reset invalidates the selection
        with pytest.raises(rt.RTError, match="rt_accum_selection"):
            b.selection()
        _masked_sequence(b)
        b.select_mask(mA ^ mB)
        b.add_selected(4)
        _same_all(a, b, "reset and the same sequence again")


# ---- 8. stream -----------------------------------------------------------------------------------------------
def test_device_entries_on_a_callers_stream(scene_of):
    import torch

    g = scene_of("p2_t05.cli")
    mA, _ = _seq_masks()
    st = torch.cuda.Stream()
    rgb = torch.zeros((CH, CW, 3), dtype=torch.float32, device="cuda")
    argb = torch.zeros((CH, CW), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((CH, CW), dtype=torch.int32, device="cuda")
    cnt0 = torch.ones((CH, CW), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as a, \
            g.accumulator(CW, CH, seed=SEED, moments=True, counts=True) as b:
        a.add(2, stream=st.cuda_stream)
        a.counts_device(cnt0.data_ptr(), stream=st.cuda_stream)  # uniform counts
        a.select_mask(mA)
        a.add_selected(3, stream=st.cuda_stream)
        a.add_selected(4, stream=st.cuda_stream)
        a.resolve_device(rgb.data_ptr(), argb.data_ptr(), stream=st.cuda_stream)
        a.counts_device(cnt.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        b.add(2)
        b.select_mask(mA)
        b.add_selected(7)
        _same_all(a, b, "a caller's stream against the scene's")
        want_rgb, want_argb = b.resolve()
        _same(rgb.cpu().numpy(), want_rgb, "resolve_device")
        assert np.array_equal(argb.cpu().numpy(), want_argb)
        assert np.array_equal(cnt.cpu().numpy(), b.counts()) and (cnt0.cpu().numpy() == 2).all()


# ---- 9. driver -----------------------------------------------------------------------------------------------
def test_driver_noise(scene_of, tmp_path):
    from PIL import Image

    cli = "c3shinyBall.cli"
    native.build()
    exe = tmp_path / "rtrender"
    subprocess.run(["g++", "-O2", "-std=c++17", str(REPO / "tools" / "rtrender.cpp"), "-o", str(exe), f"-L{native.LIB_DIR}",
                    "-ldistraytracer", "-lz", f"-Wl,-rpath,{native.LIB_DIR}"], check=True, capture_output=True)
    out = tmp_path / "n.png"
    W, H, E, TOP = 24, 20, 0.01, 32
    r = subprocess.run([str(exe), str(scenes.SCENE_DIR), cli, "-w", str(W), "-h", str(H), "-seed", str(SEED),
                        "-noise", str(E), "-max", str(TOP), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("pixels ")]
    assert len(lines) == 1 and lines[0][0::2] == ["pixels", "samples", "max"], r.stdout
    npix, total, most = (int(v) for v in lines[0][1::2])
    assert npix == W * H and most <= TOP
    g = scene_of(cli)
    with g.accumulator(W, H, seed=SEED, moments=True, counts=True) as a:  # the driver's loop
        a.add(4)
        top, chunk = 4, 4
        while a.select_error(E, TOP) > 0 and top < TOP:
            c = min(chunk, TOP - top)
            a.add_selected(c)
            top += c
            chunk = min(2 * chunk, 64)
        cnt = a.counts()
    assert total == int(cnt.sum()) and most == int(cnt.max())
    assert 4 * W * H < total < TOP * W * H  # some pixels were left alone, some were not
    img = np.asarray(Image.open(out).convert("RGB")).astype(np.uint8)
    for n in np.unique(cnt).tolist():
        want = rt.argb_to_rgb8(_render(g, cli, W, H, n)[1])
        assert np.array_equal(img[cnt == n], want[cnt == n]), n
