"""Tile scenes for the texture tests (test_textures.py on the CPU, test_gpu_textures.py on the GPU).

A tile scene holds many materials at once: one small primitive per material on a grid in the plane
z = Z0, PITCH apart, the grid centred on the z axis so that the texture coordinates take both signs
in x and y (z is negative throughout). Each tile gets RAYS rays aimed at seeded random points of it from
origins around the front light, which stands on the camera's side far enough for no tile to shadow
another. The camera of the frame tests looks down -z from the origin and sees the whole grid.

Every generator takes `only` -- "identity" keeps the tiles whose CTM is the identity or a translation
(the subset tests/golden/make_kats.py loads), None keeps all -- and overrides that re-state the same
scene with one parameter changed, for conditions decided in the oracle alone: flip_fwd (useFwdTrans
0 <-> 1 on every tile), mortar (every stone tile's threshold), short (the short argument form: no
randomised colours, so a tile's colours are its colour pairs at a fixed blend)."""
import functools
import math

import numpy as np

from tests import trace_util as tu

SEED = 20261
Z0 = -10.0
PITCH = 1.0
R = 0.35
RAYS = 96
LIGHT = (0.0, 0.0, 4.0)        # the front light; the camera is at the origin
BACK_LIGHT = (0.0, 0.0, -13.0)  # lights planar tiles seen from behind (gen_tex_image)
FAR = 300.0                    # the translated row: object-space x = world x - FAR
DIFFUSE = "diffuse .9 .9 .9 0 0 0"


class Tile:
    """One material on one primitive. mat: the lines between the `diffuse` line and the primitive;
    prim(cx, cy): the primitive's lines with the tile's centre at (cx, cy, Z0); aim_r: the radius of the
    disc through the centre (plane z = Z0) whose points the rays are aimed at; side: where its rays start."""

    def __init__(self, name, kind, mat, prim=None, aim_r=0.9 * R, side="front", **facts):
        self.name, self.kind, self.mat, self.prim, self.aim_r, self.side = name, kind, list(mat), prim or sphere, aim_r, side
        self.identity = facts.pop("identity", True)   # CTM identity or a translation
        self.moved = facts.pop("moved", False)        # CTM not the identity: useFwdTrans matters
        self.facts = facts
        self.index, self.centre = -1, None
        self.reach = facts.pop("reach", 0.5 * PITCH)


# ---- primitives -----------------------------------------------------------------------------------------
def sphere(cx, cy):
    return ["sphere %r %r %r %r" % (R, cx, cy, Z0)]


def far_sphere(cx, cy):
    """The translated row: the same world sphere under `translate FAR 0 0`, so the object-space hit
    point has x near -FAR. The second translate restores the CTM exactly (FAR - FAR = 0)."""
    return ["translate %r 0 0" % FAR, "sphere %r %r %r %r" % (R, cx - FAR, cy, Z0), "translate %r 0 0" % -FAR]


def bent_sphere(cx, cy):
    """A rotated, non-uniformly scaled sphere (an ellipsoid of semi-axes 0.39, 0.24, 0.3 in world space)."""
    return ["push", "translate %r %r %r" % (cx, cy, Z0), "rotate 30 0 1 0", "rotate 20 1 0 0", "scale 1.3 0.8 1", "sphere 0.3 0 0 0", "pop"]


# ---- material lines -------------------------------------------------------------------------------------
def perlin_line(kind, scale, octaves, turb, pd, py, fwd, colors=(25, .2), opts=None):
    """The 13-token form (11 tokens when colors is None) of marble / wood / wood2."""
    o = opts or {}
    fwd = (1 - fwd) if o.get("flip_fwd") else fwd
    tok = [kind, scale, octaves, turb, *pd, *py, fwd]
    if colors is not None and not o.get("short"):
        tok += list(colors)
    return " ".join(str(t) for t in tok)


def stone_line(scale, dist_fn, roi, npts, avg, mortar, fwd, colors=(12, .2), opts=None):
    o = opts or {}
    fwd = (1 - fwd) if o.get("flip_fwd") else fwd
    if o.get("mortar") is not None:
        mortar = o["mortar"]
    tok = ["stone", scale, dist_fn, roi, npts, repr(float(avg)), mortar, fwd]
    if colors is not None and not o.get("short"):
        tok += list(colors)
    return " ".join(str(t) for t in tok)


PERLIN_BASE = {  # scale, octaves, turbMult, periodMult, colour scale / multiplier
    "marble": (1.5, 8, 4.0, (0.6, 3.0, 1.2), (24, .1)),
    "wood": (2.0, 4, .4, (17, 3.6, 4.3), (25, .2)),
    "wood2": (1.5, 8, .4, (22, 7.9, 6.2), (25, .3)),
}
COLOR_LISTS = {
    "numeric": ["noise_color 0.1 0.3 0.2 1", "noise_color 0.9 0.7 0.3 1"],
    "named": ["noise_color named clr_darkblue", "noise_color named CLR_LightYellow 2"],
    "three": ["noise_color 0.2 0.1 0.4", "noise_color named clr_offwhite", "noise_color 1 0 0"],
}


def perlin_tiles(opts=None):
    T = [Tile("plain", "plain", []), ]
    for s in (0.5, 5, 20, 300):
        T.append(Tile("noise %s" % s, "noise", ["noise %s" % s], scale=s, big=(s == 300)))
    T.append(Tile("noise 5 far", "noise", ["noise 5"], far_sphere, moved=True, far=True, big=True, scale=5))
    for kind, (sc, oc, tb, pd, col) in PERLIN_BASE.items():
        def line(opts=opts, kind=kind, sc=sc, oc=oc, tb=tb, pd=pd, col=col, **kw):
            a = dict(scale=sc, octaves=oc, turb=tb, pd=pd, py=(0, 0, 0), fwd=0, colors=col)
            a.update(kw)
            return perlin_line(kind, a["scale"], a["octaves"], a["turb"], a["pd"], a["py"], a["fwd"], a["colors"], opts)
        add = lambda name, mat, prim=None, **f: T.append(Tile("%s %s" % (kind, name), kind, mat, prim, scale=f.pop("scale", sc), **f))  # noqa: E731
        add("defaults", [kind], scale={"marble": 1.0, "wood": 2.0, "wood2": 1.0}[kind], defaults=True)
        add("11 tokens", [line(colors=None)])
        add("13 tokens", [line()])
        add("fwd 1", [line(fwd=1)], fwd=1)
        for fwd in (0, 1):
            add("bent fwd %d" % fwd, [line(fwd=fwd)], bent_sphere, identity=False, moved=True, fwd=fwd, aim_r=0.2)
            add("far fwd %d" % fwd, [line(fwd=fwd)], far_sphere, moved=True, far=True, fwd=fwd, big=(fwd == 0))
        add("far fwd 1 scale 40", [line(fwd=1, scale=40)], far_sphere, moved=True, far=True, fwd=1, big=True, scale=40)
        for o in (1, 4, 16):
            add("octaves %d" % o, [line(octaves=o)], octaves=o)
        add("pi multipliers 0 1 0", [line(py=(0, 1, 0))])
        add("pi multipliers 1 1 1", [line(py=(1, 1, 1))])
        add("period x 0", [line(pd=(0, pd[1], pd[2]))])
        add("turbMult 0", [line(turb=0)])
        for name, cl in COLOR_LISTS.items():
            add("colours " + name, [line()] + cl)
        add("colours before the command", COLOR_LISTS["numeric"] + [line()])  # setTexture's reset forgets them
    return T


# mortar thresholds near the median ROI value of each (distance function, ROI function, numPtsDist) at one
# point per cell on average, so that a tile shows mortar and brick; from the restatement in make_kats.py
# (stone_mortar_table below prints it), checked on the oracle's output by the tests
STONE_SCALE = 6.0


def stone_mortar_table(n=160, seed=SEED):
    m = tu.make_kats()
    g = np.random.default_rng(seed)
    pts = g.random((n, 3)) * [12, 12, 4] + [-6, -6, -32]
    out = {}
    for df in (0, 1):
        for roi in range(10):
            for npts in (1, 2, 3, 8):
                ts = m.TextureState()
                ts.set_texture(stone_line(1.0, df, roi, npts, 1.0, 0.5, 0).split())
                tex = m.ProcTexture(ts)
                vals = []
                for p in pts:
                    m.TRACE.clear()
                    tex.stone(list(p))
                    vals.append([e for e in m.TRACE if e[0] == "stone"][0][2])
                out[(df, roi, npts)] = round(float(np.median(vals)), 3)
    m.TRACE.clear()
    return out


STONE_MORTAR = {
    (0, 0, 1): 0.738, (0, 0, 2): 0.579, (0, 0, 3): 0.339, (0, 0, 8): 0.092,
    (0, 1, 1): 0.738, (0, 1, 2): 0.228, (0, 1, 3): 0.84, (0, 1, 8): 0.641,
    (0, 2, 1): 0.738, (0, 2, 2): 0.308, (0, 2, 3): 0.808, (0, 2, 8): 0.482,
    (0, 3, 1): 0.738, (0, 3, 2): 0.271, (0, 3, 3): 0.642, (0, 3, 8): 0.014,
    (0, 4, 1): 0.553, (0, 4, 2): 0.123, (0, 4, 3): 0.644, (0, 4, 8): 0.289,
    (0, 5, 1): 0.738, (0, 5, 2): 0.566, (0, 5, 3): 0.281, (0, 5, 8): 0.006,
    (0, 6, 1): 0.553, (0, 6, 2): 1.0, (0, 6, 3): 1.0, (0, 6, 8): 1.0,
    (0, 7, 1): 0.738, (0, 7, 2): 0.416, (0, 7, 3): 0.323, (0, 7, 8): 0.274,
    (0, 8, 1): 0.553, (0, 8, 2): 0.303, (0, 8, 3): 0.218, (0, 8, 8): 0.1,
    (0, 9, 1): 0.738, (0, 9, 2): 0.228, (0, 9, 3): 0.84, (0, 9, 8): 0.641,
    (1, 0, 1): 0.496, (1, 0, 2): 0.826, (1, 0, 3): 0.496, (1, 0, 8): 0.135,
    (1, 1, 1): 0.496, (1, 1, 2): 0.166, (1, 1, 3): 0.632, (1, 1, 8): 0.424,
    (1, 2, 1): 0.496, (1, 2, 2): 0.389, (1, 2, 3): 0.579, (1, 2, 8): 0.55,
    (1, 3, 1): 0.496, (1, 3, 2): 0.132, (1, 3, 3): 0.556, (1, 3, 8): 0.372,
    (1, 4, 1): 0.403, (1, 4, 2): 0.099, (1, 4, 3): 0.48, (1, 4, 8): 0.234,
    (1, 5, 1): 0.496, (1, 5, 2): 0.809, (1, 5, 3): 0.638, (1, 5, 8): 0.083,
    (1, 6, 1): 0.403, (1, 6, 2): 0.92, (1, 6, 3): 1.0, (1, 6, 8): 1.0,
    (1, 7, 1): 0.496, (1, 7, 2): 0.233, (1, 7, 3): 0.163, (1, 7, 8): 0.101,
    (1, 8, 1): 0.403, (1, 8, 2): 0.225, (1, 8, 3): 0.163, (1, 8, 8): 0.076,
    (1, 9, 1): 0.496, (1, 9, 2): 0.166, (1, 9, 3): 0.632, (1, 9, 8): 0.424,
}


@functools.lru_cache(maxsize=None)
def pdf_edge_avg(cell, lo=0.3, hi=0.95):
    """An avgNumPerCell whose pdf table has the key of 2 points EQUAL to the first nextDouble of the given
    cell's generator: lowerKey (strictly below) gives that cell 1 point where floorKey or `<=` would give 2.
    Found by stepping the double nearest the solution of e^-a (1 + a + a^2 / 2) = p through its
    neighbours (the table is built as the constructor builds it). None when p is outside [lo, hi]."""
    m = tu.make_kats()
    rnd = m.JRandom()
    rnd.set_seed(m.hash_ints(*cell))
    p = rnd.next_double()
    if not lo <= p <= hi:
        return None
    f = lambda a: math.exp(-a) * (1 + a + a * a / 2) - p  # noqa: E731
    a0, a1 = 0.05, 6.0
    for _ in range(200):
        mid = 0.5 * (a0 + a1)
        a0, a1 = (mid, a1) if f(mid) > 0 else (a0, mid)
    for start, step in ((a0, math.inf), (a0, -math.inf)):
        a = start
        for _ in range(4000):
            keys = [k for k, v in m.pdf_table(a).items() if v == 2]
            if keys and keys[0] == p:
                return a
            a = math.nextafter(a, step)
    return None


def stone_tiles(opts=None):
    T = [Tile("plain", "plain", [])]
    for df in (0, 1):
        for roi in range(10):
            for npts in (1, 2, 3, 8):
                mo = STONE_MORTAR[(df, roi, npts)]
                # linLogROI is not folded back below 1: over 3 points it falls below 1 only where points are dense,
                # over 8 points never (8 log(1 + d) > 1 at any density the pdf table allows), so that tile is all brick
                avg = 15 if (roi == 6 and npts >= 3) else 1.0
                T.append(Tile("stone dist %d roi %d pts %d" % (df, roi, npts), "stone",
                              [stone_line(STONE_SCALE, df, roi, npts, avg, mo, 0, opts=opts)], scale=STONE_SCALE, dist=df,
                              roi=roi, npts=npts, mortar=mo, ncolors=10, one_sided=(roi == 6 and npts == 8)))
    add = lambda name, mat, prim=None, **f: T.append(Tile("stone " + name, "stone", mat, prim, scale=f.pop("scale", STONE_SCALE), **f))  # noqa: E731
    for avg in (0.25, 1, 4, 15):
        add("avg %s" % avg, [stone_line(STONE_SCALE, 1, 1, 2, avg, 0.1, 0, opts=opts)], mortar=0.1, ncolors=10, avg=avg)
    for mo, roi, npts in ((0, 1, 2), (0.05, 1, 2), (0.6, 0, 1), (1.5, 1, 2)):
        add("mortar %s" % mo, [stone_line(STONE_SCALE, 1, roi, npts, 1.0, mo, 0, opts=opts)], mortar=mo, ncolors=10)
    add("fwd 1", [stone_line(STONE_SCALE, 1, 1, 2, 1.0, 0.1, 1, opts=opts)], mortar=0.1, ncolors=10, fwd=1)
    for fwd in (0, 1):
        add("bent fwd %d" % fwd, [stone_line(STONE_SCALE, 1, 1, 2, 1.0, 0.1, fwd, opts=opts)], bent_sphere, identity=False,
            moved=True, fwd=fwd, aim_r=0.2, mortar=0.1, ncolors=10)
        add("far fwd %d" % fwd, [stone_line(STONE_SCALE, 0, 1, 2, 1.0, 0.1, fwd, opts=opts)], far_sphere, moved=True, far=True,
            fwd=fwd, big=(fwd == 0), mortar=0.1, ncolors=10)
    add("short form", [stone_line(STONE_SCALE, 1, 1, 2, 1.0, 0.1, 0, colors=None, opts=opts)], mortar=0.1, ncolors=10)
    add("defaults", ["stone"], scale=4.0, mortar=0.05, ncolors=10)
    cols = [(round(0.1 + 0.05 * k, 2), round(0.9 - 0.045 * k, 3), round(0.2 + 0.03 * ((k * 7) % 16), 2)) for k in range(16)]
    for n in (4, 5, 16):
        add("%d colours" % n, [stone_line(STONE_SCALE, 1, 1, 2, 1.0, 0.1, 0, opts=opts)] +
            ["noise_color %r %r %r" % c for c in cols[:n]], mortar=0.1, ncolors=n)
    # its line needs the tile's place (scene_of fills it); about one cell wide, so not held to both outcomes or two pairs
    add("pdf edge", [], mortar=0.15, ncolors=10, one_sided=True, pdf_edge=True)
    return T


def _pdf_edge_line(t, opts):
    """The `pdf edge` tile: a noise scale, a cell and an avgNumPerCell such that the cell's first draw EQUALS the
    pdf table's key of 2 points (pdf_edge_avg), and such that the second point the cell would then hold lies on
    the sphere's lit cap: the rays around it see it as their nearest point under floorKey or `<=`, and never
    under lowerKey. The scale is the first of 1.5, 1.6, ... 4.0 at which a cell near the cap has both properties."""
    m = tu.make_kats()
    c = np.asarray(t.centre)
    for s in [round(1.5 + 0.1 * k, 1) for k in range(26)]:
        base = [m.fastfloor(v) for v in (c + [0, 0, R]) * s]
        for n in m.NGHBR:
            cell = (base[0] + n[0], base[1] + n[1], base[2] + n[2])
            rnd = m.JRandom()
            rnd.set_seed(m.hash_ints(*cell))
            draws = [rnd.next_double() for _ in range(7)]  # the probability, point 1, point 2
            off = (np.asarray(cell) + draws[4:7]) / s - c
            if abs(np.linalg.norm(off) - R) > 0.03 or off[2] < 0.25:
                continue
            a = pdf_edge_avg(cell)
            if a is not None:
                t.facts.update(avg=a, edge_cell=cell, scale=s)
                return [stone_line(s, 1, 1, 2, a, 0.15, 0, opts=opts)]
    raise AssertionError("no scale puts a usable cell's second point on the pdf edge tile's cap")


# ---- image tiles ----------------------------------------------------------------------------------------
def image_textures(seed=SEED):
    """name -> uint8 [h, w, 3]: 1 x 1, 2 x 2, 1 wide x 7 high, 5 x 3, 64 x 64 random, and one all-255."""
    g = np.random.default_rng(seed + 5)
    tex = {"t%dx%d.png" % (w, h): g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
           for w, h in ((1, 1), (2, 2), (1, 7), (5, 3), (64, 64))}
    tex["white.png"] = np.full((4, 4, 3), 255, np.uint8)
    return tex


UV = ((-0.01, 0.15), (1.11, 0.15), (1.11, 0.95), (-0.17, 1.11))  # corner texture coordinates: partly outside [0, 1]
HALF = 0.4


def _poly(kind, verts):
    out = ["begin" + (" quad" if kind == "quad" else "")]
    for (x, y, z), (u, v) in verts:
        out += ["texture_coord %r %r" % (u, v), "vertex %r %r %r" % (x, y, z)]
    return out + ["end"]


def quad_corners(cx, cy):
    """No two opposite edges parallel: the reference's quad coordinates divide by |e0|^2 |e2|^2 - (e0 . e2)^2
    (myPlanarObject.java:54-62), which is 0 for a parallelogram (rect_quad below)."""
    return [(cx - HALF, cy - HALF, Z0), (cx + HALF, cy - HALF, Z0), (cx + 0.2 * HALF, cy + HALF, Z0), (cx - HALF, cy + 0.3 * HALF, Z0)]


def quad(cx, cy):
    return _poly("quad", list(zip(quad_corners(cx, cy), UV)))


def rect_quad(cx, cy):
    c = [(cx - HALF, cy - HALF, Z0), (cx + HALF, cy - HALF, Z0), (cx + HALF, cy + HALF, Z0), (cx - HALF, cy + HALF, Z0)]
    return _poly("quad", list(zip(c, UV)))


def quad_uv(t, pos, reverse=False):
    """(u, v) texture coordinates (before the texel scaling) of world points on a `quad` tile, by
    myPlanarObject.findTxtrCoords (myPlanarObject.java:178-186 with the setup of :44-62), in numpy; reverse:
    the vertex order of a quad hit from behind (invertNormal :71-88)."""
    P = np.asarray(quad_corners(t.centre[0], t.centre[1]))
    uv = np.asarray(UV)
    if reverse:
        P, uv = P[::-1], uv[::-1]
    e0, e2 = P[1] - P[0], P[3] - P[2]
    d0, d2, dn = e0 @ e0, e2 @ e2, -(e0 @ e2)
    inv = 1.0 / (d0 * d2 - dn * dn)
    v2 = pos - P[0]
    dot20, dot21 = v2 @ e0, v2 @ -e2
    cu, cv = (d2 * dot20 - dn * dot21) * inv, (d0 * dot21 - dn * dot20) * inv
    cw = 1 - cu - cv
    return uv[0, 0] * cw + uv[1, 0] * cu + uv[2, 0] * cv, uv[0, 1] * cw + uv[1, 1] * cu + uv[2, 1] * cv


def triangle(cx, cy):
    c = [(cx - HALF, cy - HALF, Z0), (cx + HALF, cy - HALF, Z0), (cx, cy + HALF, Z0)]
    return _poly("tri", list(zip(c, (UV[0], UV[1], (0.6, 1.25)))))


def tri_list(cx, cy):
    """Eight textured triangles (a tilted 2 x 2 patch of split squares) in a begin_list / end_accel BVH, plus a ninth
    far below the patch's plane: the element the root drops (Q1) is the last of the x-sorted list."""
    out = ["begin_list"]
    h = HALF / 2
    for j in range(2):
        for i in range(2):
            x0, y0 = cx - HALF + 2 * h * i, cy - HALF + 2 * h * j
            zt = lambda x, y: Z0 + 0.25 * (x - cx) + 0.125 * (y - cy)  # noqa: E731 -- tilted: a flat leaf box is never hit (Q3)
            p = [(x, y, zt(x, y)) for x, y in ((x0, y0), (x0 + 2 * h, y0), (x0 + 2 * h, y0 + 2 * h), (x0, y0 + 2 * h))]
            uv = [((q[0] - cx) / HALF, (q[1] - cy) / HALF * 0.7 + 0.4) for q in p]
            out += _poly("tri", [(p[0], uv[0]), (p[1], uv[1]), (p[2], uv[2])])
            out += _poly("tri", [(p[0], uv[0]), (p[2], uv[2]), (p[3], uv[3])])
    out += _poly("tri", [((cx + HALF + 0.02, cy, Z0 - 0.01), (0, 0)), ((cx + HALF + 0.04, cy, Z0 - 0.01), (1, 0)),
                         ((cx + HALF + 0.03, cy + 0.01, Z0 - 0.01), (0, 1))])
    return out + ["end_accel"]


def image_tiles(opts=None):
    tex = lambda n: ["texture " + n]  # noqa: E731
    T = [Tile("plain", "plain", [])]
    for n in ("t1x1.png", "t2x2.png", "t1x7.png", "t5x3.png", "t64x64.png", "white.png"):
        T.append(Tile("sphere " + n, "image", tex(n), sphere, sphere=True, tex=n, nan=(n == "t1x1.png")))  # 0 / 0 at height 1
    T.append(Tile("sphere far", "image", tex("t5x3.png"), far_sphere, moved=True, sphere=True, tex="t5x3.png"))
    T.append(Tile("ellipsoid", "image", tex("t64x64.png"),
                  lambda cx, cy: ["ellipsoid 0.35 0.2 0.3 %r %r %r" % (cx, cy, Z0)], aim_r=0.17, identity=False))
    T.append(Tile("bent sphere", "image", tex("t64x64.png"), bent_sphere, identity=False, moved=True, aim_r=0.2))
    T.append(Tile("sphereIn", "image", tex("t64x64.png"),
                  lambda cx, cy: ["point_light %r %r %r 1 1 1" % (cx, cy, Z0), "sphereIn %r %r %r %r" % (R, cx, cy, Z0)],
                  side="inside", identity=False))
    T.append(Tile("moving sphere", "image", tex("t64x64.png"),
                  lambda cx, cy: ["moving_sphere %r %r %r %r %r %r %r" % (R, cx - 0.1, cy, Z0, cx + 0.1, cy, Z0)],
                  aim_r=0.2, identity=False))
    T.append(Tile("quad front", "image", tex("t5x3.png"), quad, aim_r=0.6 * HALF, planar=True, identity=False))
    T.append(Tile("quad back", "image", tex("t5x3.png"), quad, aim_r=0.6 * HALF, side="back", planar=True, identity=False))
    T.append(Tile("quad 1 wide", "image", tex("t1x7.png"), quad, aim_r=0.6 * HALF, planar=True, identity=False))
    T.append(Tile("quad 64", "image", tex("t64x64.png"), quad, aim_r=0.6 * HALF, planar=True, identity=False))
    T.append(Tile("triangle", "image", tex("t64x64.png"), triangle, aim_r=0.12, identity=False))
    T.append(Tile("triangle back", "image", tex("t5x3.png"), triangle, aim_r=0.12, side="back", identity=False))
    T.append(Tile("quad parallelogram", "image", tex("t5x3.png"), rect_quad, aim_r=HALF, identity=False, nan=True))
    T.append(Tile("bvh triangles", "image", tex("t64x64.png"), tri_list, aim_r=0.9 * HALF, identity=False))
    T.append(Tile("bvh triangles back", "image", tex("t5x3.png"), tri_list, aim_r=0.9 * HALF, side="back", identity=False))
    T.append(Tile("cylinder", "image", tex("t2x2.png"),
                  lambda cx, cy: ["cylinder 0.3 %r %r %r %r" % (cx, Z0, cy - 0.3, cy + 0.3)], aim_r=0.25, identity=False))
    T.append(Tile("box", "image", tex("t2x2.png"),
                  lambda cx, cy: ["box %r %r %r %r %r %r" % (cx - 0.3, cy - 0.3, Z0 - 0.3, cx + 0.3, cy + 0.3, Z0 + 0.3)],
                  aim_r=0.25, identity=False))
    inst = lambda shdr: (lambda cx, cy: ["push", "translate %r %r %r" % (cx, cy, Z0), "scale 0.35 0.3 0.35",  # noqa: E731
                                         "instance ball" + (" shdr" if shdr else ""), "pop"])
    T.append(Tile("instance", "image", tex("t5x3.png"), inst(False), identity=False, aim_r=0.25))
    T.append(Tile("instance shdr", "image", tex("t2x2.png"), inst(True), identity=False, aim_r=0.25))
    T.append(Tile("plane", "image", tex("t5x3.png"), lambda cx, cy: ["plane 0 0 1 14"], aim_r=0.45, identity=False, plane=True, nan=True))
    return T


IMAGE_HEAD = [DIFFUSE, "texture t64x64.png", "sphere 1 0 0 0", "named_object ball"]  # the instances' base, textured 64 x 64


# ---- scenes ---------------------------------------------------------------------------------------------
class TileScene:
    def __init__(self, name, text, tiles, cols, rows, textures):
        self.name, self.text, self.tiles, self.cols, self.rows, self.textures = name, text, tiles, cols, rows, textures
        self.fov = 2 * math.degrees(math.atan((max(cols, rows) * PITCH / 2 + 0.1) / -Z0))

    def rays(self, seed=SEED, n=RAYS):
        """(origin [m, 3], direction [m, 3], tile index [m]): n rays per tile in tile order."""
        g = np.random.default_rng(seed)
        os_, ds, ids = [], [], []
        for t in self.tiles:
            rad = t.aim_r * np.sqrt(g.random(n))
            ang = g.random(n) * 2 * math.pi
            z = -14.0 if t.facts.get("plane") else Z0
            target = np.stack([t.centre[0] + rad * np.cos(ang), t.centre[1] + rad * np.sin(ang), np.full(n, z)], 1)
            if t.side == "inside":
                o = np.asarray(t.centre) + (g.random((n, 3)) - 0.5) * 0.1
                d = g.normal(size=(n, 3))
            else:
                o = np.asarray(LIGHT if t.side == "front" else BACK_LIGHT) + (g.random((n, 3)) - 0.5) * 0.4
                d = target - o
            os_.append(o)
            ds.append(d)
            ids.append(np.full(n, t.index))
        return np.concatenate(os_), np.concatenate(ds), np.concatenate(ids)

    def pole_rays(self):
        """For every tile with the fact `sphere`: one ray aimed exactly at the pole that faces the z axis (the
        lit one: sin(v pi) = 0 there, the |b1| < EPS branch of findTextureU), and five at the point of the
        z = centre seam nearest the axis, moved by 0, +-1e-8 and +-2e-7 in z (z1 <= EPS and its neighbours,
        myImpObject.java:97-109). Returns (origin, direction, tile index, kind) with kind "pole" / "seam"."""
        os_, ds, ids, kinds = [], [], [], []
        for t in self.tiles:
            if not t.facts.get("sphere"):
                continue
            c = np.asarray(t.centre)
            s = -1.0 if c[1] > 0 else 1.0
            pole = c + [0, s * R, 0]
            os_.append(pole + 5 * np.array([0, s * 0.3, 1.0]))
            ds.append(pole - os_[-1])
            ids.append(t.index)
            kinds.append("pole")
            hyp = math.hypot(c[0], c[1])
            inward = -np.array([c[0], c[1], 0.0]) / hyp if hyp > 0 else np.array([1.0, 0, 0])
            for dz in (0.0, 1e-8, -1e-8, 2e-7, -2e-7):
                q = c + R * inward + [0, 0, dz]
                os_.append(q + 5 * (0.3 * inward + [0, 0, 1.0]))
                ds.append(q - os_[-1])
                ids.append(t.index)
                kinds.append("seam")
        return np.array(os_), np.array(ds), np.array(ids), np.array(kinds)

    def on_tile(self, pos, hit):
        """Tile index of each hit position (-1: none): within the tile's reach of its centre."""
        out = np.full(len(pos), -1)
        for t in self.tiles:
            c = np.array([t.centre[0], t.centre[1], -14.0 if t.facts.get("plane") else Z0])
            out[hit & (np.linalg.norm(pos - c, axis=1) < t.reach)] = t.index
        return out


def scene_of(name, tiles, opts, only, head=(), textures=None, back_light=False):
    if only == "identity":
        tiles = [t for t in tiles if t.identity]
    n = len(tiles)
    cols = math.ceil(math.sqrt(n))
    rows = math.ceil(n / cols)
    L = ["fov %r" % (2 * math.degrees(math.atan((max(cols, rows) * PITCH / 2 + 0.1) / -Z0))), "background 0 0 0",
         "point_light %r %r %r 1 1 1" % LIGHT]
    if back_light:
        L.append("point_light %r %r %r 1 1 1" % BACK_LIGHT)
    L += list(head) if only != "identity" else []   # the instances' base object
    for i, t in enumerate(tiles):
        t.index = i
        t.centre = ((i % cols - (cols - 1) / 2) * PITCH, ((rows - 1) / 2 - i // cols) * PITCH, Z0)
        if t.facts.get("pdf_edge"):
            t.mat = _pdf_edge_line(t, opts)
        L.append("diffuse .6 .5 .4 0 0 0" if t.kind == "plain" else DIFFUSE)
        L += t.mat
        L += t.prim(t.centre[0], t.centre[1])
    return TileScene(name, "\n".join(L) + "\n", tiles, cols, rows, textures or {})


def gen_tex_perlin(only=None, **opts):
    return scene_of("gen_tex_perlin", perlin_tiles(opts), opts, only)


def gen_tex_stone(only=None, **opts):
    return scene_of("gen_tex_stone", stone_tiles(opts), opts, only)


def gen_tex_image(only=None, **opts):
    return scene_of("gen_tex_image", image_tiles(opts), opts, only, head=IMAGE_HEAD, textures=image_textures(), back_light=True)


GENERATORS = {"gen_tex_perlin": gen_tex_perlin, "gen_tex_stone": gen_tex_stone, "gen_tex_image": gen_tex_image}


# ---- one scene on the oracle, and the conditions that keep a comparison from passing on nothing ------------
FIRST_KEY = 5000


def clean(rgb):
    """NaN channels (the reference's 0 / 0 texture coordinates) as -1, so that they compare as values."""
    return np.where(np.isnan(rgb), -1.0, rgb)


class OracleCase:
    """A tile scene loaded by the oracle with its rays (the tiles' rays, then the pole and seam rays), the
    oracle's closest-hit records and its colours for samples 0 and 3, computed once."""

    def __init__(self, gen, d, only=None):
        from oracle.oracle import OracleScene

        self.gen, self.dir, self.only = gen, d, only
        self.sc = gen(only=only)
        self.cli = self.sc.name + ("_identity" if only else "") + ".cli"
        (d / self.cli).write_text(self.sc.text)
        self.o = OracleScene(d, self.cli, self.sc.textures)
        o, dd, tid = self.sc.rays()
        po, pd, ptid, kinds = self.sc.pole_rays() if any(t.facts.get("sphere") for t in self.sc.tiles) else (o[:0], dd[:0], tid[:0], tid[:0].astype(str))
        self.origin, self.dir_, self.tile = np.concatenate([o, po]), np.concatenate([dd, pd]), np.concatenate([tid, ptid])
        self.family = np.concatenate([np.full(len(o), "tile"), kinds])
        self.rec = self.o.trace(self.origin, self.dir_, seed=SEED, first_key=FIRST_KEY)
        self.on = self.sc.on_tile(self.rec["pos"], self.rec["hit"])
        self.want = {s: self.o.shade(self.origin, self.dir_, seed=SEED, first_key=FIRST_KEY, sample=s) for s in (0, 3)}

    def variant(self, **opts):
        """The oracle's sample-0 colours of the same rays in the scene re-stated with opts."""
        from oracle.oracle import OracleScene

        sc = self.gen(only=self.only, **opts)
        assert [t.centre for t in sc.tiles] == [t.centre for t in self.sc.tiles]
        name = self.cli[:-4] + "_" + "_".join("%s_%s" % kv for kv in sorted(opts.items())) + ".cli"
        (self.dir / name).write_text(sc.text)
        o = OracleScene(self.dir, name, sc.textures)
        rgb, _ = o.shade(self.origin, self.dir_, seed=SEED, first_key=FIRST_KEY)
        o.close()
        return rgb

    def close(self):
        self.o.close()


def _chroma(rgb):
    return np.unique(np.round(rgb[:, :2] / rgb.sum(1, keepdims=True), 6), axis=0)


def check_conditions(c):
    """Asserted on the oracle's output alone. Returns a dict of figures for the test to print."""
    sc, rec = c.sc, c.rec
    rgb = c.want[0][0]
    fam_tile = c.family == "tile"
    lit = np.nan_to_num(rgb, nan=1.0).sum(1) > 0
    fig = {}
    stone = [t for t in sc.tiles if t.kind == "stone"]
    if stone:
        brick_all, mortar_all = c.variant(mortar=0.0), c.variant(mortar=2.0)
        pairs = c.variant(mortar=0.0, short=1)
    fwd_tiles = [t for t in sc.tiles if "fwd" in t.facts]
    flipped = c.variant(flip_fwd=1) if fwd_tiles else None
    for t in sc.tiles:
        m = fam_tile & (c.tile == t.index)
        own = m & (c.on == t.index)
        assert own.sum() >= 48, (t.name, int(own.sum()))                          # hit by at least 48 of its rays
        if t.facts.get("nan"):
            assert np.isnan(rgb[own]).all(), t.name                              # the reference's 0 / 0 coordinates
            continue
        assert not np.isnan(rgb[m]).any() or t.facts.get("planar") or t.facts.get("plane"), t.name
        if t.kind != "plain":
            ncol = len(np.unique(rgb[own & lit & ~np.isnan(rgb).any(1)], axis=0))
            assert ncol >= 20, (t.name, ncol)                                    # at least 20 distinct colours
        if t.kind == "stone":
            use = own & lit
            is_brick, is_mortar = (rgb[use] == brick_all[use]).all(1), (rgb[use] == mortar_all[use]).all(1)
            assert (is_brick | is_mortar).all(), t.name
            mo = t.facts["mortar"]
            if 0 < mo <= 1 and not t.facts.get("one_sided"):
                assert is_brick.any() and is_mortar.any(), (t.name, int(is_brick.sum()), int(is_mortar.sum()))
            elif mo <= 0:
                assert is_brick.all(), t.name
            elif mo > 1:
                assert is_mortar.all(), t.name
            if t.facts["ncolors"] >= 6 and not t.facts.get("pdf_edge"):
                assert len(_chroma(pairs[use])) >= 2, (t.name, _chroma(pairs[use]))   # two brick pairs
        if flipped is not None:
            differs = (rgb[own & lit] != flipped[own & lit]).any(1)
            if t.moved and "fwd" in t.facts:
                assert differs.mean() > 0.5, (t.name, float(differs.mean()))
            elif not t.moved:
                assert not differs.any(), t.name
        if t.facts.get("big"):                                                   # scaled coordinates beyond 256
            p = rec["pos"][own] - ([FAR, 0, 0] if t.facts.get("far") and not t.facts.get("fwd") else [0, 0, 0])
            top = float(np.abs(p * t.facts["scale"]).max())
            fig[t.name + " |scaled coordinate|"] = top
            assert top > 256, (t.name, top)
        if t.facts.get("planar"):                                                # (u, v) outside and inside [0, 1]
            rev = rec["args"][own] == 0 if t.side == "back" else rec["args"][own] == 1
            u0, v0 = quad_uv(t, rec["pos"][own], reverse=False)
            u1, v1 = quad_uv(t, rec["pos"][own], reverse=True)
            u, v = np.where(rev, u1, u0), np.where(rev, v1, v0)
            outside = (u < 0) | (u > 1) | (v < 0) | (v > 1)
            # a negative texel coordinate (the truncating cast, a negative blend weight, the index clamp): u < 0 or v > 1
            assert outside.sum() >= 10 and (~outside).sum() >= 10 and ((u < 0) | (v > 1)).sum() >= 5, (t.name, int(outside.sum()))
        if t.facts.get("sphere"):
            ex = (c.tile == t.index) & ~fam_tile
            centre = np.asarray(t.centre)
            pole = ex & (c.family == "pole")
            assert pole.sum() == 1 and c.on[pole][0] == t.index
            assert np.abs(np.abs(rec["pos"][pole][0] - centre) - [0, R, 0]).max() < 1e-9, t.name
            z1 = rec["pos"][ex & (c.family == "seam")][:, 2] - Z0
            assert (z1 <= 1e-7).sum() >= 2 and (z1 > 1e-7).sum() >= 1 and (c.on[ex] == t.index).all(), (t.name, z1)
            assert lit[ex].all(), t.name
    assert len(c.origin) == len(rgb) == len(c.tile)
    return fig
