"""Shared pieces of the ray-query tests (test_trace_abi.py, test_gpu_trace.py): generated scene texts
within the subset tests/golden/make_kats.py restates (fov, background, point_light, shaders,
translate, sphere, polygons, begin_list / end_accel), the adversarial ray families F1-F4, camera
rays, and the plain-Python reference records (computed once per scene and shared)."""
import functools
import importlib.util
import math
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
SEED = 20260


@functools.lru_cache(maxsize=None)
def make_kats():
    spec = importlib.util.spec_from_file_location("make_kats", GOLDEN / "make_kats.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- generated scenes ------------------------------------------------------------------------------
# Coordinates are multiples of 1/64 (exact in decimal and binary), scaled scenes print repr().
def _tri_lines(tris, scale):
    out = []
    for t in tris:
        out.append("begin")
        for v in t:
            out.append("vertex %r %r %r" % tuple(float(x) * scale for x in v))
        out.append("end")
    return out


def random_tris(n=150, seed=SEED):
    """n small triangles in the cube [-1, 1]^3 (grid 1/64): centre + three offsets of up to 0.3."""
    g = np.random.default_rng(seed)
    c = g.integers(-45, 46, size=(n, 1, 3))
    off = g.integers(-19, 20, size=(n, 3, 3))
    return (c + off) / 64.0


def coplanar_tris(seed=SEED):
    """Axis-aligned coplanar clusters: 8 clusters of 12 triangles, each cluster in one plane
    x / y / z = const, so its leaf boxes have zero extent along that axis (Q3)."""
    g = np.random.default_rng(seed + 1)
    tris = []
    for k in range(8):
        axis = k % 3
        plane = int(g.integers(-40, 41))
        cen = g.integers(-40, 41, size=3)
        for _ in range(12):
            t = cen + g.integers(-12, 13, size=(3, 3))
            t[:, axis] = plane
            tris.append(t)
    return np.asarray(tris) / 64.0


GROUND = np.array([[[-100, -1.5, -100], [100, -1.5, 100], [100, -1.5, -100]],
                   [[100, -1.5, 100], [-100, -1.5, -100], [-100, -1.5, 100]]], dtype=np.float64)
SPHERE = (0.5, (1.75, 0.25, -2.5))  # radius, centre (scene b)
SHIFT = (0.0, 0.0, -3.0)            # translate of the BVH


def scene_text(kind="a", scale=1.0):
    """kind a: two ground triangles + a 150-triangle BVH under `translate 0 0 -3` (triangles only);
    b: a + a sphere with a transparent `shiny` material (the transparent kernel variant);
    coplanar: the ground + the coplanar clusters as the BVH. scale multiplies every coordinate."""
    tris = coplanar_tris() if kind == "coplanar" else random_tris()
    L = ["fov 60", "background 0.1 0.1 0.2", "point_light %r %r %r .8 .8 .8" % (3 * scale, 4 * scale, 0.0),
         "diffuse .8 .8 .8 .2 .2 .2"]
    L += _tri_lines(GROUND, scale)
    if kind == "b":
        L.append("shiny .8 .8 .8 .2 .2 .2 .5 .5 .5 20 0.3 0.6")
        L.append("sphere %r %r %r %r" % (SPHERE[0] * scale, *(c * scale for c in SPHERE[1])))
        L.append("diffuse .7 .5 .3 .1 .1 .1")
    L.append("translate %r %r %r" % tuple(c * scale for c in SHIFT))
    L.append("begin_list")
    L += _tri_lines(tris, scale)
    L.append("end_accel")
    return "\n".join(L) + "\n"


def bvh_world_tris(kind="a", scale=1.0):
    """World-space triangles [n, 3, 3] of a generated scene's BVH."""
    tris = coplanar_tris() if kind == "coplanar" else random_tris()
    return (tris + np.asarray(SHIFT)) * scale


# ---- rays ------------------------------------------------------------------------------------------
def camera_rays(W, H, fov):
    """The un-jittered 1-spp FOV camera rays, row-major (myFOVScene.draw :1498-1508)."""
    view_z = -1 * (max(H, W) / 2.0) / math.tan((math.pi * fov / 180.0) / 2)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([col - W / 2.0, -1 * (row - H / 2.0), np.full((H, W), view_z)], -1).reshape(-1, 3)
    return np.zeros_like(d), d


def _nudge(x, k):
    """x moved by k ulps (k int array in [-4, 4])."""
    x = x.copy()
    for s in range(1, 5):
        up, dn = k >= s, k <= -s
        x[up] = np.nextafter(x[up], np.inf)
        x[dn] = np.nextafter(x[dn], -np.inf)
    return x


def families(tris, n, seed=SEED):
    """The adversarial families over world triangles tris [m, 3, 3]: {name: (o [n, 3], d [n, 3])}.
    F1 origins at vertices nudged 0..+-4 ulps per coordinate, aimed at random root-box points;
    F2 exactly axis-aligned directions (+-0.0 in the other components) from outside and inside the box;
    F3 origins on a root-box face plane +-4 ulps, aimed inward; F4 from outside, aimed exactly at
    vertices and edge midpoints."""
    g = np.random.default_rng(seed)
    verts = tris.reshape(-1, 3)
    lo, hi = verts.min(0), verts.max(0)
    ext = hi - lo
    ext = np.where(ext > 0, ext, np.abs(hi).max() * 0.01 + 1e-300)
    inside = lambda m: lo + g.random((m, 3)) * (hi - lo)  # noqa: E731
    out = {}
    # F1
    o = _nudge(verts[g.integers(0, len(verts), n)], g.integers(-4, 5, size=(n, 3)))
    out["F1"] = (o, inside(n) - o)
    # F2
    axis = g.integers(0, 3, n)
    sign = g.choice([-1.0, 1.0], n)
    d = np.where(g.random((n, 3)) < 0.5, 0.0, -0.0)
    d[np.arange(n), axis] = sign
    o = inside(n)
    outside = np.arange(n) < n // 2  # the first half starts outside the box, before the face it points at
    start = np.where(sign > 0, lo[axis] - ext[axis] * (0.25 + g.random(n)), hi[axis] + ext[axis] * (0.25 + g.random(n)))
    o[outside, axis[outside]] = start[outside]
    out["F2"] = (o, d)
    # F3
    axis = g.integers(0, 3, n)
    side = g.integers(0, 2, n)
    o = inside(n)
    o[np.arange(n), axis] = _nudge(np.where(side == 0, lo[axis], hi[axis]), g.integers(-4, 5, size=n))
    out["F3"] = (o, inside(n) - o)
    # F4
    e = g.integers(0, 3, n)
    tri = tris[g.integers(0, len(tris), n)]
    a, b = tri[np.arange(n), e], tri[np.arange(n), (e + 1) % 3]
    target = np.where((g.random(n) < 0.5)[:, None], a, (a + b) * 0.5)
    u = g.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (lo + hi) * 0.5 + u * np.linalg.norm(ext) * 2.0
    out["F4"] = (o, target - o)
    return out


def incoherent_rays(tris, n, seed=SEED):
    """Random rays: origins in a shell around the root box, aimed at random points of the box grown by half."""
    g = np.random.default_rng(seed + 7)
    verts = tris.reshape(-1, 3)
    lo, hi = verts.min(0), verts.max(0)
    u = g.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (lo + hi) * 0.5 + u * np.linalg.norm(hi - lo) * (0.2 + 1.3 * g.random((n, 1)))
    target = lo - 0.25 * (hi - lo) + g.random((n, 3)) * 1.5 * (hi - lo)
    return o, target - o


def reference_rays(kind):
    """The ~4 k rays of the full-record comparison: 1 k incoherent + 768 of each family."""
    tris = bvh_world_tris(kind)
    fam = families(tris, 768, seed=SEED + 3)
    os_, ds = [incoherent_rays(tris, 1024)[0]], [incoherent_rays(tris, 1024)[1]]
    for k in ("F1", "F2", "F3", "F4"):
        os_.append(fam[k][0])
        ds.append(fam[k][1])
    return np.concatenate(os_), np.concatenate(ds)


# ---- the plain-Python reference ------------------------------------------------------------------
def creation_order(sc):
    """{id(object): index into rt_scene_desc.prims} of a make_kats scene: objects are created in
    file order, a list's members before the objects after its end_accel."""
    order, n = {}, 0
    for obj in sc.objs:
        for o in (obj.members if hasattr(obj, "members") else [obj]):
            order[id(o)] = n
            n += 1
    return order


def load_reference(kind):
    """(make_kats module, scene, reset). The restatement keeps the reference's object state: a planar
    object re-normalises its normal in place on every hit (myPlanarObject.java:132-133), a
    history-dependent last-ulp drift the product does not reproduce (both
    implementations use the first-hit value). reset() puts every object a query touched back into its
    never-hit state (_setup() recomputes N and D from the current vertex order), so each query sees
    first-hit values whatever came before it."""
    m = make_kats()
    sc = m.load(scene_text(kind), 64, 64)
    touched = []
    for obj in sc.objs:
        for o in (obj.members if hasattr(obj, "members") else [obj]):
            if hasattr(o, "v"):
                o.v_file = [list(p) for p in o.v]  # the file's vertex order: a ray from behind reverses it

                def normal_at(pt, args, _o=o, _orig=o.normal_at):
                    touched.append(_o)
                    return _orig(pt, args)
                o.normal_at = normal_at

    def reset():
        for o in touched:
            o._setup()
        touched.clear()
    return m, sc, reset


HIT_FIELDS = ("hit", "prim", "top", "args", "in_accel", "t", "pos", "normal")
TMAX = (3.0, 8.0, math.inf)


@functools.lru_cache(maxsize=None)
def reference_records(kind):
    """findClosestRayHit / calcShadow of reference_rays(kind) by tests/golden/make_kats.py: a dict of
    arrays (HIT_FIELDS; occ [len(TMAX), n]) plus `gap`, the smallest relative difference between a
    ray's best and second-best candidate t over every object of the scene (inf: fewer than two)."""
    m, sc, reset = load_reference(kind)
    order = creation_order(sc)
    top_of = {id(o): i for i, o in enumerate(sc.objs)}
    o, d = reference_rays(kind)
    n = len(o)
    rec = {"hit": np.zeros(n, bool), "prim": np.full(n, -1), "top": np.full(n, -1), "args": np.zeros(n, int),
           "in_accel": np.zeros(n, bool), "t": np.full(n, np.inf), "pos": np.zeros((n, 3)), "normal": np.zeros((n, 3)),
           "occ": np.zeros((len(TMAX), n), np.uint8), "gap": np.full(n, np.inf)}
    for i in range(n):
        # a fresh myRay per query (the traversal re-normalises its direction in place)
        best, best_top = None, -1
        ray = m.Ray(o[i], d[i], 0)
        for ti, obj in enumerate(sc.objs):  # Scene.closest, keeping the winning objList index
            h = obj.intersect(ray, ray.transformed(obj.ctm[1]), obj.ctm)
            if h is not None and (best is None or h.t < best.t):
                best, best_top = h, ti
        if best is not None:
            ob = best.obj
            rec["hit"][i] = True
            rec["prim"][i] = order[id(ob)]
            rec["top"][i] = best_top
            rec["in_accel"][i] = id(ob) not in top_of
            rec["args"][i] = int(hasattr(ob, "v") and ob.v != ob.v_file)  # planar orientation bit; spheres 0
            rec["t"][i] = best.t
            rec["pos"][i] = best.fwd_hit
            rec["normal"][i] = best.nrm
        reset()
        for j, tm in enumerate(TMAX):
            rec["occ"][j, i] = 1 if sc.shadowed(m.Ray(o[i], d[i], 0), tm) else 0
            reset()
    rec["gap"] = candidate_gap(kind, o, d, rec["t"])
    return rec


def candidate_gap(kind, o, d, best_t):
    """Per ray, the smallest relative difference between best_t and any OTHER candidate t: every
    object of the scene (list members one by one, the BVH's dropped element included, no box tests),
    by the restatement's formulas vectorised in numpy -- plane t = -(N . o + D) / (N . d), t > 1e-7,
    an inside test that accepts a superset (edge functions >= -1e-6 |N|^2), the sphere's nearer
    root above 1e-7. A superset of candidates only lowers the gap. inf where there is no other."""
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    tris = np.concatenate([GROUND, bvh_world_tris(kind)])
    v0, v1, v2 = tris[:, 0], tris[:, 1], tris[:, 2]
    N = np.cross(v1 - v0, v2 - v0)  # [m, 3]
    with np.errstate(all="ignore"):
        pr = dn @ N.T  # [n, m]
        t = ((N * v0).sum(1)[None, :] - o @ N.T) / pr
        p = o[:, None, :] + t[..., None] * dn[:, None, :]  # [n, m, 3]
        ok = (t > 1e-7) & np.isfinite(t)
        nn = (N * N).sum(1)
        for a, b in ((v0, v1), (v1, v2), (v2, v0)):
            e = np.cross(b - a, p - a)  # edge function x N
            ok &= (e * N).sum(-1) >= -1e-6 * nn
        ts = [np.where(ok, t, np.inf)]
        if kind == "b":
            r, c = SPHERE
            oc = o - np.asarray(c)
            bq = (dn * oc).sum(1)
            disc = bq * bq - ((oc * oc).sum(1) - r * r)
            sq = np.sqrt(np.where(disc >= 0, disc, np.nan))
            t1, t2 = -bq - sq, -bq + sq
            tsph = np.where(t1 > 1e-7, t1, np.where(t2 > 1e-7, t2, np.inf))
            ts.append(np.where(np.isnan(tsph), np.inf, tsph)[:, None])
        T = np.concatenate(ts, 1)
        # drop each ray's own winner: the candidate nearest to best_t
        own = np.argmin(np.abs(T - best_t[:, None]), 1)
        T[np.arange(len(T)), own] = np.inf
        gap = np.abs(T - best_t[:, None]) / np.maximum(np.abs(T), np.abs(best_t[:, None]))
        gap = np.where(np.isfinite(T), gap, np.inf).min(1)
    return np.where(np.isfinite(best_t), gap, np.inf)
