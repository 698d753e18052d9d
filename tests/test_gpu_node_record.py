"""The packet traversals' record reads (trace_kernels.h sload_nodef / sload_trif / sload_tri as whole-record
loads, the nearest-first pop taking the pending child's reference from its frame): the triangles-only
kernels (variant F = 0) against the per-lane all-fp64 traversal of the same kernels (`TRACE_LANES`), bit for
bit in every field of the closest-hit record and in occlusion, and 32 x 32 frames against the all-features
kernel, which keeps the field-by-field loads and the pop's own load.

The scenes are the smallest that reach each path. The builder splits a BVH at the median of `n - 1` members
(the reference drops the last one) and makes a leaf of five or fewer (scene_build.cpp bvh), so:

  leaf_root   2 triangles: the accel's root is a leaf, no node record is read;
  two_leaves  7 triangles, the fewest with an internal node: one node, both children leaf-run references;
  mixed       300 random triangles: node and leaf children mixed, pushes and pops on every level;
  deep        400,000 small triangles along the z axis: 17 nested internal levels, one more than the LDS levels
              of the packet stack (PK_LDS = 16), so rays along the axis push and pop frames past them. The depth
              is a function of the count alone with a median split (triangles of growing size do not deepen
              it), which is why this scene is as large as it is; its depth is asserted;
  huge        the 150-triangle scene of tests/trace_util.py scaled by 1e30: the fp32 margins overflow and the
              pre-tests settle nothing.

Rays: incoherent rays and the adversarial families of tests/trace_util.py over each BVH's triangles -- F2 has
exactly axis-aligned directions with signed zeros in the other components, from outside and inside the root
box, F1 and F3 start inside child boxes (on vertices and on root-box face planes, nudged by ulps)."""
import numpy as np
import pytest

from distraytracer_old_amd import rt
from tests import trace_util as tu
from tests.test_gpu_trace import _same_bits

pytestmark = pytest.mark.gpu

SEED = tu.SEED
FIELDS = ("flags", "prim", "top", "args", "material", "t", "pos", "normal")
TMAX = (3.0, 8.0, np.inf)
SHIFT = np.asarray(tu.SHIFT)
DEEP_N = 400_000
DEEP_STEP = 1.0 / 64


def deep_tris(n=DEEP_N):
    """n triangles of half-width 1/64 .. 3/64 strung along -z, one per 1/64, each tilted a little."""
    i = np.arange(n)
    a = (1 + i % 3) / 64.0
    z = -(i + 1) * DEEP_STEP
    t = np.zeros((n, 3, 3))
    t[:, 0] = np.stack([-a, -a, z], 1)
    t[:, 1] = np.stack([a, -a, z], 1)
    t[:, 2] = np.stack([np.zeros(n), a, z + (i % 5 - 2) / 1024.0], 1)
    return t


def bvh_tris(name):
    """Object-space triangles of scene `name`'s BVH and the scale of the whole scene."""
    if name == "leaf_root":
        return tu.random_tris(2, SEED + 21), 1.0
    if name == "two_leaves":
        return tu.random_tris(7, SEED + 22), 1.0
    if name == "mixed":
        return tu.random_tris(300, SEED + 23), 1.0
    if name == "deep":
        return deep_tris(), 1.0
    assert name == "huge"
    return tu.random_tris(), 1e30


NAMES = ("leaf_root", "two_leaves", "mixed", "deep", "huge")
# (internal nodes, depth of the deepest leaf) the builder reports for each scene
SHAPE = {"leaf_root": (0, 0), "two_leaves": (1, 1), "deep": (None, 17)}


def scene_text(name):
    tris, scale = bvh_tris(name)
    L = ["fov 60", "background 0.1 0.1 0.2", "point_light %r %r %r .8 .8 .8" % (3 * scale, 4 * scale, 0.0), "diffuse .8 .8 .8 .2 .2 .2"]
    L += tu._tri_lines(tu.GROUND, scale)
    L += ["diffuse .7 .5 .3 .1 .1 .1", "translate %r %r %r" % tuple((SHIFT * scale).tolist()), "begin_list"]
    if len(tris) > 10000:  # the large scene: formatted in one pass (multiples of 1/1024, exact in decimal)
        L.append("\n".join(map("begin\nvertex %r %r %r\nvertex %r %r %r\nvertex %r %r %r\nend".__mod__, map(tuple, tris.reshape(-1, 9).tolist()))))
    else:
        L += tu._tri_lines(tris, scale)
    L.append("end_accel")
    return "\n".join(L) + "\n"


def build_rays(name):
    tris, scale = bvh_tris(name)
    world = (tris + SHIFT) * scale
    if name == "deep":
        # along the axis, both ways, through the triangles and through the corners of their boxes (those miss
        # every triangle and visit every leaf); then rays across the string
        g = np.random.default_rng(SEED + 24)
        n = 384
        xy = (g.random((n, 2)) * 2 - 1) * 2.5 / 64
        far = world[:, :, 2].min() - 1.0
        o = np.concatenate([np.column_stack([xy[: n // 2], np.full(n // 2, 1.0)]), np.column_stack([xy[n // 2:], np.full(n - n // 2, far)])])
        d = np.zeros((n, 3))
        d[: n // 2, 2], d[n // 2:, 2] = -1.0, 1.0
        d[::4, :2] = (g.random((len(d[::4]), 2)) * 2 - 1) * 1e-6  # one in four a little off the axis
        oc, dc = tu.incoherent_rays(world[:: DEEP_N // 512], 256)
        return np.concatenate([o, oc]), np.concatenate([d, dc])
    fam = tu.families(world, 384, seed=SEED + 25)
    oi, di = tu.incoherent_rays(world, 768)
    return np.concatenate([oi] + [fam[k][0] for k in ("F1", "F2", "F3", "F4")]), np.concatenate([di] + [fam[k][1] for k in ("F1", "F2", "F3", "F4")])


@pytest.fixture(scope="module")
def scene_of(tmp_path_factory):
    d = tmp_path_factory.mktemp("node_record")
    cache = {}

    def get(name):
        if name not in cache:
            (d / f"{name}.cli").write_text(scene_text(name))
            cache[name] = rt.Scene.load_cli(f"{name}.cli", scene_dir=d, textures={})
        return cache[name], cache[name].info()

    yield get
    for s in cache.values():
        s.close()


@pytest.mark.parametrize("name", NAMES)
def test_packet_against_lanes_and_default_against_generic(name, scene_of):
    s, info = scene_of(name)
    assert s.variant() == (0, 0)
    print(name, {k: info[k] for k in ("triangles", "bvh_internal", "bvh_leaves", "bvh_depth")})
    if name in SHAPE:
        internal, depth = SHAPE[name]
        assert info["bvh_depth"] == depth and (internal is None or info["bvh_internal"] == internal)
    if name == "deep":
        assert info["bvh_depth"] > 16  # frames past the packet stack's 16 LDS levels
    if name == "mixed":
        assert info["bvh_internal"] > 30 and info["bvh_depth"] >= 5
    o, d = build_rays(name)
    want = s.trace(o, d, seed=SEED, flags=rt.TRACE_LANES)
    got = s.trace(o, d, seed=SEED)
    hits = int(((want["flags"] & rt.HIT_HIT) != 0).sum())
    in_accel = int(((want["flags"] & rt.HIT_IN_ACCEL) != 0).sum())
    print(name, "rays", len(o), "hits", hits, "in the BVH", in_accel)
    assert in_accel >= {"leaf_root": 50, "two_leaves": 50, "deep": 150}.get(name, 200)
    assert not _same_bits(got, want, fields=FIELDS)
    gen = s.trace(o, d, seed=SEED, flags=rt.TRACE_GENERIC)
    assert not _same_bits(got, gen, fields=FIELDS)
    scale = bvh_tris(name)[1]
    for tm in TMAX:
        a = s.occluded(o, d, tm * scale, seed=SEED)
        b = s.occluded(o, d, tm * scale, seed=SEED, flags=rt.TRACE_LANES)
        assert np.array_equal(a, b), (tm, int((a != b).sum()))
        if tm == np.inf:
            assert (a == 1).sum() >= 50
    ra, aa = s.render(32, 32, spp=2, seed=SEED)
    rb, ab = s.render(32, 32, spp=2, seed=SEED, flags=rt.RENDER_GENERIC)
    assert np.array_equal(aa, ab) and np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
