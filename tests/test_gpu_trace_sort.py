"""RT_TRACE_SORT on the GPU: a batch reordered for coherence on the device returns the same bytes as the
batch traced in the caller's order, and rt_trace_order shows the order it ran in.

1. Same bytes: seven scenes (generated ones, one scaled by 1e5, coplanar clusters, a moving sphere whose
   ray time hangs on the ray's key, instances, C3's 69 k-triangle BVH), shuffled camera rays, incoherent
   rays and the adversarial families, closest hit and occlusion, four traversal modes.
2. Tails: batch sizes around the wave size.
3. Rejected and degenerate rays: rejected rays keep their own index and sort last; every ray rejected;
   identical origins; origins with components of 1e300 and 1e-310.
4. The order: deterministic, a permutation, and it restores the coherence of a shuffled camera frame.
5. Windows (DISTRAYTRACER_SORT_WINDOW) and staging chunks are sorted independently.
6. Scratch growth on one scene, and the device entries on a side stream."""
import numpy as np
import pytest

from distraytracer_old_amd import desc, rt, scenes
from tests import trace_util as tu

pytestmark = pytest.mark.gpu

SORT = rt.TRACE_SORT
MODES = {"packet": 0, "lanes": rt.TRACE_LANES, "nocull": rt.TRACE_NOCULL, "generic": rt.TRACE_GENERIC}
GENERATED = {"gen_a": ("a", 1.0), "gen_b": ("b", 1.0), "gen_coplanar": ("coplanar", 1.0), "gen_a_large": ("a", 1e5)}
SAME_BYTES = ["gen_a", "gen_b", "gen_coplanar", "gen_a_large", "p2_t03.cli", "p3_t02.cli", "c3_bun69k.cli"]


@pytest.fixture(scope="module")
def gen_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("trace_sort_scenes")
    for name, (kind, scale) in GENERATED.items():
        (d / f"{name}.cli").write_text(tu.scene_text(kind, scale))
    return d


def _load(name, gen_dir):
    if name in GENERATED:
        return rt.Scene.load_cli(f"{name}.cli", scene_dir=gen_dir, textures={})
    return rt.Scene.load_cli(name)


@pytest.fixture(scope="module")
def scene_of(gen_dir):
    """name -> a loaded scene (kept for the module: one upload per scene)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _load(name, gen_dir)
        return cache[name]

    yield get
    for s in cache.values():
        s.close()


def _fov(name):
    if name in GENERATED:
        return 60.0
    for line in (scenes.SCENE_DIR / name).read_text().splitlines():
        t = line.split()
        if t and t[0] == "fov":
            return float(t[1])
    raise AssertionError(name)


def _shuffled_camera(W, fov, seed):
    o, d = tu.camera_rays(W, W, fov)
    perm = np.random.default_rng(seed).permutation(W * W)
    return o[perm], d[perm], perm


def _is_perm(order, lo, hi):
    return order.dtype == np.uint32 and np.array_equal(np.sort(order.astype(np.int64)), np.arange(lo, hi))


def _diff(a, b):
    """Indices of the records whose bytes differ (the first few)."""
    x = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    y = np.ascontiguousarray(b).view(np.uint8).reshape(len(b), -1)
    return np.flatnonzero((x != y).any(1))[:8].tolist()


def _assert_sorted_equals_unsorted(g, o, d, what, modes=MODES, tmaxes=(3.0, np.inf), **key):
    for mode, fl in modes.items():
        want = g.trace(o, d, flags=fl, **key)
        got = g.trace(o, d, flags=fl | SORT, **key)
        assert got.tobytes() == want.tobytes(), (what, mode, "closest", _diff(got, want))
        for tmax in tmaxes:
            want_occ = g.occluded(o, d, tmax, flags=fl, **key)
            got_occ = g.occluded(o, d, tmax, flags=fl | SORT, **key)
            assert got_occ.tobytes() == want_occ.tobytes(), (what, mode, tmax, _diff(got_occ, want_occ))


# ---- 1. same bytes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SAME_BYTES)
def test_sorted_trace_returns_the_same_bytes(name, scene_of):
    g = scene_of(name)
    o, d, _ = _shuffled_camera(64, _fov(name), seed=3)
    batches = {"camera": (o, d)}
    if name in GENERATED:
        tris = tu.bvh_world_tris(*GENERATED[name])
        batches["incoherent"] = tu.incoherent_rays(tris, 4096)
        batches.update(tu.families(tris, 1024))
    key = dict(seed=0, first_key=0)
    if name == "p2_t03.cli":  # the moving sphere's ray time hangs on the key: a slot-keyed ray would show here
        key = dict(seed=77, first_key=12345)
        a, b = g.trace(o, d, **key), g.trace(o, d, seed=77, first_key=0)
        assert len(_diff(a, b)) >= 1
    for bname, (bo, bd) in batches.items():
        hit = (g.trace(bo, bd, **key)["flags"] & rt.HIT_HIT) != 0
        print(name, bname, len(bo), "rays, hit share", float(hit.mean()))
        _assert_sorted_equals_unsorted(g, bo, bd, (name, bname), **key)
    assert ((g.trace(o, d, **key)["flags"] & rt.HIT_HIT) != 0).any()


# ---- 2. tails --------------------------------------------------------------------------------------
def test_batch_sizes_around_the_wave_size(scene_of):
    g = scene_of("gen_a")
    o, d = tu.incoherent_rays(tu.bvh_world_tris("a"), 4097, seed=11)
    for n in (1, 63, 64, 65, 127, 4097):
        _assert_sorted_equals_unsorted(g, o[:n], d[:n], n, modes={"packet": 0, "lanes": rt.TRACE_LANES}, seed=1, first_key=9)
        assert _is_perm(g.trace_order(o[:n], d[:n]), 0, n), n


# ---- 3. rejected and degenerate rays ------------------------------------------------------------------
def _gen_a_rays(n=1024):
    o, d = tu.incoherent_rays(tu.bvh_world_tris("a"), n, seed=21)
    return o.copy(), d.copy(), np.full(n, np.inf)


def _spoil(o, d, tmax, idx):
    """Make the rays idx rejected ones, cycling through NaN origin, Inf direction, zero direction, NaN tmax."""
    for j, i in enumerate(idx):
        k = j % 4
        if k == 0:
            o[i, j % 3] = np.nan
        elif k == 1:
            d[i, j % 3] = np.inf if j % 8 < 4 else -np.inf
        elif k == 2:
            d[i] = [0.0, -0.0, 0.0]
        else:
            tmax[i] = np.nan


def _traces(g, o, d, tmax, flags=0):
    r = rt.rays(o, d, tmax)  # through rt_trace_rays itself: Scene.trace does not pass tmax on
    import ctypes
    n = len(r)
    hits, occ = np.zeros(n, dtype=desc.HIT_DTYPE), np.zeros(n, dtype=np.uint8)
    p = desc.TraceParams(0, 0, flags, 0)
    assert rt.lib().rt_trace_rays(g._h, ctypes.byref(p), r.ctypes.data, n, hits.ctypes.data, None) == 0
    p = desc.TraceParams(0, 0, flags | rt.TRACE_ANY, 0)
    assert rt.lib().rt_trace_rays(g._h, ctypes.byref(p), r.ctypes.data, n, None, occ.ctypes.data) == 0
    return hits, occ


def test_rejected_rays_keep_their_index_and_sort_last(scene_of):
    g = scene_of("gen_a")
    o, d, tmax = _gen_a_rays()
    good, good_occ = _traces(g, o, d, tmax)
    bad = np.arange(0, 1024, 7)
    _spoil(o, d, tmax, bad)
    is_bad = np.zeros(1024, bool)
    is_bad[bad] = True
    for fl in (0, rt.TRACE_LANES):
        want, want_occ = _traces(g, o, d, tmax, fl)
        got, got_occ = _traces(g, o, d, tmax, fl | SORT)
        assert got.tobytes() == want.tobytes() and got_occ.tobytes() == want_occ.tobytes()
        assert np.array_equal((got["flags"] & rt.HIT_BAD_RAY) != 0, is_bad) and np.array_equal(got_occ == 2, is_bad)
        assert (got["flags"][is_bad] == rt.HIT_BAD_RAY).all()
        assert got[~is_bad].tobytes() == good[~is_bad].tobytes() and np.array_equal(got_occ[~is_bad], good_occ[~is_bad])
    order = g.trace_order(o, d, tmax)
    assert _is_perm(order, 0, 1024)
    assert np.array_equal(np.sort(order[-len(bad):]), bad)  # the rejected rays fill the last slots


def _degenerate(case):
    o, d, tmax = _gen_a_rays()
    if case == "all rejected":
        _spoil(o, d, tmax, np.arange(1024))
    elif case == "identical origins":
        o[:] = [0.25, 0.5, 1.0]
    else:  # finite extremes: the bounds span 2e300, a denormal beside them
        o[5, 0], o[9, 1], o[11, 2] = 1e300, -1e300, 1e-310
        o[12] = [1e300, -1e300, 1e-310]
        o[13] = [-1e300, 1e300, -1e-310]
    return o, d, tmax


@pytest.mark.parametrize("case", ["all rejected", "identical origins", "extreme origins"])
def test_degenerate_batches(case, scene_of):
    g = scene_of("gen_a")
    o, d, tmax = _degenerate(case)
    order = g.trace_order(o, d, tmax)
    assert _is_perm(order, 0, 1024), case
    want, want_occ = _traces(g, o, d, tmax)
    got, got_occ = _traces(g, o, d, tmax, SORT)
    assert got.tobytes() == want.tobytes() and got_occ.tobytes() == want_occ.tobytes(), case
    if case == "all rejected":
        assert (got["flags"] == rt.HIT_BAD_RAY).all() and (got_occ == 2).all()
    else:
        assert not (got["flags"] & rt.HIT_BAD_RAY).any()
    if case == "extreme origins":  # and extreme directions, through the key alone
        d[14], d[15], d[16] = [1e300, -1e300, 1e-310], [1e-310, 0.0, -1e-310], [0.0, 0.0, -5e-324]
        assert _is_perm(g.trace_order(o, d, tmax), 0, 1024)


# ---- 4. the order ----------------------------------------------------------------------------------
def _median_group_area(pixels, W):
    g = pixels.reshape(-1, 64)
    row, col = g // W, g % W
    return float(np.median((np.ptp(row, axis=1) + 1) * (np.ptp(col, axis=1) + 1)))


def test_order_is_deterministic_and_restores_coherence(scene_of):
    g = scene_of("gen_a")
    W = 128
    o, d, perm = _shuffled_camera(W, 60.0, seed=1)
    order = g.trace_order(o, d)
    assert _is_perm(order, 0, W * W)
    assert np.array_equal(order, g.trace_order(o, d))
    shuffled, srt = _median_group_area(perm, W), _median_group_area(perm[order], W)
    print("median pixel bounding box of a wave: shuffled", shuffled, "sorted", srt)
    assert srt <= shuffled / 16.0, (shuffled, srt)


# ---- 5. windows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,win", [({"DISTRAYTRACER_SORT_WINDOW": "256"}, 256),
                                     ({"DISTRAYTRACER_SORT_WINDOW": "256", "DISTRAYTRACER_TRACE_CHUNK": "512"}, 256),
                                     ({"DISTRAYTRACER_SORT_WINDOW": "300"}, 256),  # rounded down to a multiple of 64
                                     ({"DISTRAYTRACER_TRACE_CHUNK": "512"}, 512)],
                         ids=["window", "window+chunk", "rounded", "chunk"])
def test_windows_are_sorted_independently(env, win, gen_dir, scene_of, monkeypatch):
    n = 1000
    o, d = tu.incoherent_rays(tu.bvh_world_tris("a"), n, seed=31)
    g = scene_of("gen_a")
    want, want_occ = g.trace(o, d, seed=2, first_key=500), g.occluded(o, d, 3.0, seed=2, first_key=500)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with _load("gen_a", gen_dir) as c:
        got, got_occ = c.trace(o, d, seed=2, first_key=500, flags=SORT), c.occluded(o, d, 3.0, seed=2, first_key=500, flags=SORT)
        order = c.trace_order(o, d)
    assert got.tobytes() == want.tobytes() and got_occ.tobytes() == want_occ.tobytes()
    for lo in range(0, n, win):
        hi = min(lo + win, n)
        assert _is_perm(order[lo:hi], lo, hi), (lo, hi)


# ---- 6. scratch growth and streams ---------------------------------------------------------------------
def test_scratch_growth_and_the_device_entries(gen_dir, scene_of):
    import torch

    tris = tu.bvh_world_tris("b")
    o, d = tu.incoherent_rays(tris, 65536, seed=41)
    ref = scene_of("gen_b")
    want, want_occ = ref.trace(o, d, seed=3, first_key=11), ref.occluded(o, d, 8.0, seed=3, first_key=11)
    dev = torch.device("cuda", 0)
    with _load("gen_b", gen_dir) as g:
        for n in (4096, 65536, 64):  # the scratch grows, then serves a smaller batch
            got = g.trace(o[:n], d[:n], seed=3, first_key=11, flags=SORT)
            got_occ = g.occluded(o[:n], d[:n], 8.0, seed=3, first_key=11, flags=SORT)
            assert got.tobytes() == want[:n].tobytes() and got_occ.tobytes() == want_occ[:n].tobytes(), n
        n = 5000
        r = rt.rays(o[:n], d[:n], 8.0)
        t_rays = torch.from_numpy(r.view(np.uint8).reshape(-1)).to(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            t_hits = torch.zeros(n * desc.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            t_occ = torch.full((n,), 7, dtype=torch.uint8, device=dev)
            t_order = torch.zeros(n, dtype=torch.int32, device=dev)
            g.trace_device(t_rays.data_ptr(), n, hits_ptr=t_hits.data_ptr(), stream=side.cuda_stream, seed=3, first_key=11,
                           flags=SORT)
            g.trace_device(t_rays.data_ptr(), n, occ_ptr=t_occ.data_ptr(), stream=side.cuda_stream, seed=3, first_key=11,
                           flags=SORT | rt.TRACE_ANY)
            g.trace_order_device(t_rays.data_ptr(), n, t_order.data_ptr(), stream=side.cuda_stream)
        side.synchronize()
        assert t_hits.cpu().numpy().view(desc.HIT_DTYPE).tobytes() == want[:n].tobytes()
        assert np.array_equal(t_occ.cpu().numpy(), want_occ[:n])
        order = t_order.cpu().numpy().view(np.uint32)
        assert _is_perm(order, 0, n) and np.array_equal(order, g.trace_order(o[:n], d[:n], 8.0))
