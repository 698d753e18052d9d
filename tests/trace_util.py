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


# ---- every primitive type: generated scenes, ray families (test_oracle_rays.py, test_gpu_prims.py) ---
# `/` stands for a line break. Every material has its own diffuse colour.
GEN_PRIMS = """
fov 60
background 0.1 0.1 0.2
point_light 3 5 1 .7 .7 .7
spotlight -3 6 -2  0.3 -1 -0.3  20 45  .4 .4 .4
diffuse .6 .6 .6 .1 .1 .1
plane 0 1 0 1.5
diffuse .8 .2 .2 .1 .1 .1
push / translate -2 0 -6 / rotate 30 0 1 0 / rotate 20 1 0 0 / scale 1 1.5 0.5
box -0.5 -0.5 -0.5 0.5 0.5 0.5
pop
diffuse .2 .8 .2 .1 .1 .1
ellipsoid 0.6 0.3 0.4  0 0.5 -5
diffuse .2 .2 .8 .1 .1 .1
push / translate 2 -0.5 -6 / rotate 40 0 0 1
hollow_cylinder 0.5 0 0 -0.75 0.75
pop
diffuse .8 .8 .2 .1 .1 .1
push / translate 1.5 1.5 -7 / rotate -25 1 0 0 / scale 1.5 1 1
cyl 0.4 1.2 0 -0.6 0
pop
shiny .8 .8 .8 .2 .2 .2 .5 .5 .5 20 0.3 0.6
sphere 0.5 -0.75 -0.5 -3.5
reflective .3 .3 .6 .1 .1 .1 0.5
cylinder 0.4 -3 -8 -1.5 0.5
diffuse .8 .4 .8 .1 .1 .1
moving_sphere 0.4 -1.5 1.5 -5 -1.0 1.75 -5
diffuse .3 .7 .7 .1 .1 .1
sphereIn 0.5 0.75 -1 -4
diffuse .7 .5 .3 .1 .1 .1
push / translate 0 0 -9
begin_list
sphere 0.5 -1 0 0
push / rotate 15 0 0 1 / scale 2 1 1
begin quad / vertex -0.5 1 0 / vertex 0.5 1 0 / vertex 0.5 2 0 / vertex -0.5 2 0 / end
pop
cyl 0.3 1 1 -1 0
begin / vertex 2 -1 0 / vertex 3 -1 0 / vertex 2.5 1 0.5 / end
end_list
pop
diffuse .9 .9 .9 .1 .1 .1
sphere 1 0 0 0
named_object ball
push / translate -3 2 -8 / scale 0.5 0.8 0.5
instance ball
pop
diffuse .9 .5 .1 .1 .1 .1
push / translate 3 2.5 -8 / rotate 30 0 0 1 / scale 0.7 0.3 0.7
instance ball shdr
pop
"""
# creation order (rt_scene_desc.prims): the type of each primitive, and the face arguments it can report
# (the plane reports 0 only: its reversed vertex order gives the same normal again, so the reference never
# accepts a ray from behind it, oracle.cpp Planar::pick)
GEN_PRIMS_TYPES = ["plane", "box", "ellipsoid", "hollow_cylinder", "cyl", "sphere", "cylinder", "moving_sphere", "sphereIn",
                   "list sphere", "list quad", "list cyl", "list triangle", "instanced sphere"]
GEN_PRIMS_ARGS = {0: {0}, 1: {0, 1, 2, 3, 4, 5}, 3: {0, 1}, 4: {0, 1, 2}, 6: {0, 1, 2}, 10: {0, 1}, 11: {0, 1, 2}, 12: {0, 1}}
GEN_PRIMS_CLOSED = (1, 2, 3, 4, 5, 6, 8)  # family I starts inside these: box, ellipsoid, both cylinder kinds, glass, sphereIn


def gen_prims_text(disk_light=False):
    """GEN_PRIMS as .cli text; disk_light: the point light replaced by a disk light (keyed shadow points)."""
    t = "\n".join(p.strip() for line in GEN_PRIMS.strip().splitlines() for p in line.split("/")) + "\n"
    if disk_light:
        assert "point_light 3 5 1 .7 .7 .7" in t
        t = t.replace("point_light 3 5 1 .7 .7 .7", "disk_light 3 5 1 0.5 -0.4 -1 -0.2 .7 .7 .7")
    return t


def shell_rays(n, seed=SEED):
    """Family R: origins on the upper half-shell of radius 6 to 9 around (0, -1, -6) (one in eight on the
    lower one), aimed at uniform points of [-3.5, 3.5] x [-1.5, 3] x [-10, -3]."""
    g = np.random.default_rng(seed + 11)
    u = g.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[:, 1] = np.abs(u[:, 1])
    u[::8, 1] *= -1.0  # one in eight starts below the plane: planar objects seen from behind
    o = np.array([0.0, -1.0, -6.0]) + u * (6.0 + 3.0 * g.random((n, 1)))
    lo, hi = np.array([-3.5, -1.5, -10.0]), np.array([3.5, 3.0, -3.0])
    return o, lo + g.random((n, 3)) * (hi - lo) - o


def bounce_rays(o, d, rec):
    """Family B: from the hit positions of (o, d) exactly, along the mirror direction about the hit normal
    (the t > 1e-7 rule on the surface just left). Returns (o, d, index of the parent ray)."""
    i = np.flatnonzero(rec["hit"])
    dn = d[i] / np.linalg.norm(d[i], axis=1, keepdims=True)
    n = rec["normal"][i]
    return rec["pos"][i].copy(), dn - 2.0 * (dn * n).sum(1, keepdims=True) * n, i


def inside_rays(trace, o, d, rec, closed, per_prim=96, seed=SEED):
    """Family I: origins inside the closed primitives, random directions. A ray of (o, d) that enters
    primitive p is continued from its hit position (trace: the oracle's closest hit); where the
    continuation hits p again, the midpoint of the two positions lies inside p (between the two walls of
    the hollow cylinder). Returns (o, d, the primitive each origin lies inside)."""
    g = np.random.default_rng(seed + 13)
    sel = np.flatnonzero(rec["hit"] & np.isin(rec["prim"], closed))
    nxt = trace(rec["pos"][sel], d[sel])
    ok = nxt["hit"] & (nxt["prim"] == rec["prim"][sel])
    os_, of = [], []
    for p in closed:
        k = np.flatnonzero(ok & (rec["prim"][sel] == p))[:per_prim]
        os_.append(0.5 * (rec["pos"][sel][k] + nxt["pos"][k]))
        of.append(np.full(len(k), p))
    oi = np.concatenate(os_)
    u = g.normal(size=(len(oi), 3))
    return oi, u / np.linalg.norm(u, axis=1, keepdims=True), np.concatenate(of)


BAD_RAYS = {3: ("o", 0, np.nan), 64: ("o", 2, np.inf), 65: ("d", 1, -np.inf), 100: ("d", 0, np.nan), 127: ("zero", 0, 0.0),
            128: ("o", 1, -np.inf), 200: ("zero", 0, -0.0), 299: ("d", 2, np.inf)}


def spoil(o, d, table=BAD_RAYS):
    """The rejection table of test_gpu_trace.test_rejected_rays_leave_their_neighbours_unchanged applied to
    copies of o, d (at least 300 rays): returns (o, d, is_bad)."""
    o, d = o.copy(), d.copy()
    for i, (what, c, v) in table.items():
        if what == "zero":
            d[i] = [v, 0.0, -0.0]
        else:
            (o if what == "o" else d)[i, c] = v
    is_bad = np.zeros(len(o), bool)
    is_bad[list(table)] = True
    return o, d, is_bad


def gen_inst_text():
    """What instances add: a named 40-triangle BVH instanced three times under rotations and non-uniform
    scales (once with `shdr`), an instanced cyl and quad, a list holding an instance beside plain members,
    and a sierpinski of depth 2 over a named sphere. Every material has its own diffuse colour."""
    L = ["fov 60", "background 0.1 0.1 0.2", "point_light 3 5 1 .7 .7 .7", "diffuse .6 .6 .6 .1 .1 .1"]
    L += _tri_lines(GROUND, 1.0)
    L += ["diffuse .8 .2 .2 .1 .1 .1", "begin_list"] + _tri_lines(random_tris(40, SEED + 5), 1.5) + ["end_accel", "named_object mesh"]
    L += "push / translate -2 0 -6 / rotate 30 0 1 0 / scale 1 1.5 0.5 / instance mesh / pop".split(" / ")
    L += "push / translate 0.5 1 -7 / rotate 50 1 0 0 / scale 0.7 0.7 1.3 / instance mesh / pop".split(" / ")
    L += "diffuse .2 .8 .2 .1 .1 .1 / push / translate 2.5 0 -6 / rotate -40 0 0 1 / scale 1.2 0.6 1 / instance mesh shdr / pop".split(" / ")
    L += "diffuse .2 .2 .8 .1 .1 .1 / cyl 0.4 1.2 0 -0.6 0 / named_object tube".split(" / ")
    L += "push / translate -1 -0.5 -4 / rotate 35 0 0 1 / scale 1 1 1.5 / instance tube / pop".split(" / ")
    L += ("diffuse .8 .8 .2 .1 .1 .1 / begin quad / vertex -0.5 -0.5 0 / vertex 0.5 -0.5 0 / vertex 0.5 0.5 0 / vertex -0.5 0.5 0 / end"
          " / named_object card").split(" / ")
    L += "push / translate 1.5 -0.5 -4.5 / rotate 20 0 1 0 / scale 1.5 1 1 / instance card / pop".split(" / ")
    L += "diffuse .9 .9 .9 .1 .1 .1 / sphere 1 0 0 0 / named_object ball".split(" / ")
    L += ("diffuse .8 .4 .8 .1 .1 .1 / push / translate 0 2 -9 / begin_list / sphere 0.5 -1.5 0 0"
          " / push / translate 0.5 0 0 / scale 0.5 0.8 0.5 / instance ball / pop"
          " / begin / vertex 1.5 -1 0 / vertex 2.5 -1 0 / vertex 2 1 0.5 / end / end_list / pop").split(" / ")
    L += "diffuse .3 .7 .7 .1 .1 .1 / push / translate -3 2.5 -8 / sierpinski ball 2 0.5 / pop".split(" / ")
    return "\n".join(L) + "\n"


# ---- family T: rays tangent to every sphere, ellipsoid and cylinder side, through their CTMs ---------
def _rot(ang, ax, ay, az):
    """Right-handed rotation by ang degrees about (ax, ay, az), 4 x 4 (Rodrigues)."""
    a = np.array([ax, ay, az], dtype=np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(ang)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    return M


def quadrics(text):
    """The spheres, ellipsoids and cylinder sides of a generated scene with the matrix that takes each
    to world space: its own CTM (a list member is intersected through its own CTM), or the named object's
    CTM times the stack for an instance (the sierpinski's elements included). A dict per object:
    kind 'ell' (c, rad[3]) or 'cyl' (c = (x, y0, z), rad = (r, height)), M [4, 4], name, listed (a member
    of a list / BVH). The moving
    sphere is left out: its centre depends on the ray's key (moving_sphere_tangents)."""
    stack, out, named, last, listed = [np.eye(4)], [], {}, [None], [False]

    def mul(M):
        stack[-1] = stack[-1] @ M

    def tr(x, y, z):
        M = np.eye(4)
        M[:3, 3] = (x, y, z)
        mul(M)

    def add(kind, c, rad, name):
        out.append({"kind": kind, "c": np.asarray(c, float), "rad": np.asarray(rad, float), "M": stack[-1].copy(), "name": name,
                    "listed": listed[0]})
        last[0] = len(out) - 1

    def instance(name):
        for q in named.get(name, []):
            out.append({**q, "M": q["M"] @ stack[-1], "name": "instance of " + q["name"], "listed": listed[0]})

    def sierp(dim, sc, name, level, depth):  # buildSierpSubTri's layout, float constants as floats
        if level >= depth:
            return
        f = np.float32
        stack.append(stack[-1].copy())
        tr(0, float(f(0.1) * f(dim)), 0)
        mul(_rot(70, 0, 1, 0))
        instance(name)
        stack.pop()
        shift = float(f(math.sqrt(f(6.0))) / f(6.0) * f(dim))
        for k in range(4):
            stack.append(stack[-1].copy())
            if k == 0:
                tr(0, shift, 0)
            else:
                if k > 1:
                    mul(_rot(120 if k == 2 else -120, 0, 1, 0))
                mul(_rot(120, 1, 0, 0)); tr(0, shift, 0); mul(_rot(-120, 1, 0, 0))
                if k > 1:
                    mul(_rot(-120 if k == 2 else 120, 0, 1, 0))
            S = np.diag([sc, sc, sc, 1.0])
            mul(S)
            sierp(float(f(sc) * f(dim)), sc, name, level + 1, depth)
            stack.pop()

    for line in text.splitlines():
        t = line.split()
        if not t:
            continue
        c, v = t[0], [float(x) for x in t[1:] if x.replace(".", "", 1).replace("-", "", 1).isdigit()]
        if c == "begin_list":
            listed[0] = True
        elif c == "push":
            stack.append(stack[-1].copy())
        elif c == "pop":
            stack.pop()
        elif c == "translate":
            tr(*v)
        elif c == "scale":
            mul(np.diag([*v, 1.0]))
        elif c == "rotate":
            mul(_rot(*v))
        elif c in ("sphere", "sphereIn"):
            add("ell", v[1:4], [v[0]] * 3, c)
        elif c == "ellipsoid":
            add("ell", v[3:6], v[0:3], c)
        elif c == "cyl":
            add("cyl", v[2:5], (v[0], v[1]), c)
        elif c in ("cylinder", "hollow_cylinder"):
            add("cyl", (v[1], v[3], v[2]), (v[0], v[4] - v[3]), c)
        elif c in ("end", "end_accel", "end_list", "box", "plane", "moving_sphere"):
            last[0] = None  # the latest object is no quadric
            listed[0] = listed[0] and c not in ("end_accel", "end_list")
        elif c == "named_object":
            named[t[1]] = [out.pop(last[0])] if last[0] is not None else []
            last[0] = None
        elif c == "instance":
            instance(t[1])
        elif c == "sierpinski":
            listed[0] = True  # its elements are members of one BVH
            sierp(8.0, float(np.float32(t[3])), t[1], 0, int(t[2]))
            listed[0] = False
    return out


def tangent_rays(q, n, g, shift=0.0):
    """n rays tangent to quadric q (a surface point p and a tangent direction w in object space, both
    taken to world space by q's matrix; origin p - s w, s in [0.5, 2.5]). Returns (o, d, p); shift moves
    the origins along the world normal by that length (test conditions: < 0 cuts the surface near p, > 0
    passes it by)."""
    M, L = q["M"], q["M"][:3, :3]
    if q["kind"] == "ell":
        u = g.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        po, no = q["c"] + u * q["rad"], u / q["rad"]
    else:
        a = g.random(n) * 2 * np.pi
        r, h = q["rad"]
        cs = np.stack([np.cos(a), np.zeros(n), np.sin(a)], 1)
        po = q["c"] + r * cs + np.stack([np.zeros(n), h * (0.05 + 0.9 * g.random(n)), np.zeros(n)], 1)
        no = cs
    wo = np.cross(no, g.normal(size=(n, 3)))
    p = po @ L.T + M[:3, 3]
    w = wo @ L.T
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    nw = no @ np.linalg.inv(L)  # L^-T n
    nw /= np.linalg.norm(nw, axis=1, keepdims=True)
    o = p - w * (0.5 + 2.0 * g.random((n, 1))) + shift * nw
    return o, w, p


def moving_sphere_tangents(trace, prim, c0, c1, n, g, steps=70):
    """Tangent rays of a moving sphere, whose centre depends on the time drawn from ray i's key: each
    ray's direction is bisected, in its own slot i (trace(o, d) keys ray i as the final batch will),
    between an aim at the middle of the centre's path (inside the sphere at any time, since the path is
    shorter than the radius) and an aim one unit off it, down to neighbouring doubles of the
    interpolation parameter. Returns (o, d, converged mask)."""
    c0, c1 = np.asarray(c0, float), np.asarray(c1, float)
    mid = 0.5 * (c0 + c1)
    u = g.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[:, 1] = np.abs(u[:, 1])
    o = mid + u * (1.5 + g.random((n, 1)))
    off = np.cross(u, g.normal(size=(n, 3)))
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    lo, hi = np.zeros(n), np.ones(n)
    wins = lambda lam: (lambda r: r["hit"] & (r["prim"] == prim))(trace(o, mid + lam[:, None] * off - o))  # noqa: E731
    ok = wins(lo) & ~wins(hi)
    for _ in range(steps):
        m = 0.5 * (lo + hi)
        w = wins(m)
        lo, hi = np.where(w, m, lo), np.where(w, hi, m)
    ok &= (hi - lo) <= 4 * np.spacing(hi)
    lam = np.where(g.random(n) < 0.5, lo, hi)
    return o, mid + lam[:, None] * off - o, ok
