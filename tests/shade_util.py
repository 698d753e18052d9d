"""The shading space between "a hit" and "a colour" (light_sum, pow_shade, refl_dir, trans_split, the
shading tree): small generated scenes, each named for the branches it is built to reach, their caller
rays, and the plain-Python restatement (tests/golden/make_kats.py) run ray by ray with the branches it
took. tests/test_shade_space.py proves on the CPU that every fixture reaches its branches and that each
branch moves the colour; tests/test_gpu_shade_space.py then holds the kernels to the oracle on them.

Vocabulary: fov, background, the three light commands, diffuse / reflective / shiny / surface, push /
pop / translate, sphere, begin / vertex / end, begin_list / end_accel -- what the restatement parses.

Ray families, under keys first_key = FIRST_KEY + i: R from the camera position towards the objects, I
starting inside each closed sphere, N aimed within a degree of a sphere's centre.

The reference's reader gives every material a grey KReflClr (setSurface and `krefl` call
setKRefl(k, k, k, k), myScene.java:823,852), so the mirror weight of `mirrors` is a grey 0.85 / 0.9: no
command writes a coloured one."""
import functools
import math

import numpy as np

from tests import trace_util as tu

SEED = 77
FIRST_KEY = 1000
SAMPLES = (0, 3)
NUM_RAYS = 8  # myScene.numRays: a node of generation >= NUM_RAYS - 2 has no children
GATE = NUM_RAYS - 2
CAM = np.array([0.0, 0.3, 0.5])

HEAD = ["fov 60", "background 0.2 0.3 0.5"]
FLOOR = ["begin", "vertex -9 -1 -13", "vertex 9 -1 3", "vertex 9 -1 -13", "end",
         "begin", "vertex 9 -1 3", "vertex -9 -1 -13", "vertex -9 -1 3", "end"]
GREY = ["diffuse .7 .7 .7 .1 .1 .1"] + FLOOR


def _text(*parts):
    return "\n".join(line for p in parts for line in ([p] if isinstance(p, str) else p)) + "\n"


def _sphere(r, c):
    return "sphere %r %r %r %r" % (r, *c)


def _unit(g, n):
    u = g.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def make_rays(spheres, seed, n_r=2048, n_i=1024, n_n=1024, boxes=(), spots=(), per_spot=24, spot_jitter=0.02):
    """(o, d, family) of one fixture: at most 4096 rays. spheres: [(radius, centre)]; boxes: extra target
    regions [(lo, hi)] for family R (the floor under the objects is always one); spots: points that
    per_spot of the R rays are aimed at from CAM itself, within spot_jitter (highlights)."""
    g = np.random.default_rng(seed)
    regions = [(np.array([-4.5, -1.0, -9.5]), np.array([4.5, -1.0, -2.0]))] + [(np.asarray(a, float), np.asarray(b, float)) for a, b in boxes]
    ns = len(spheres)
    if ns == 0:
        n_r, n_i, n_n = n_r + n_i + n_n, 0, 0
    # R
    o_r = CAM + (g.random((n_r, 3)) - 0.5) * 0.4
    pick = g.integers(0, ns + len(regions), n_r) if ns else ns + g.integers(0, len(regions), n_r)
    tgt = np.zeros((n_r, 3))
    for k, (r, c) in enumerate(spheres):
        m = pick == k
        tgt[m] = np.asarray(c) + _unit(g, int(m.sum())) * r * 1.15 * g.random((int(m.sum()), 1)) ** (1 / 3)
    for k, (lo, hi) in enumerate(regions):
        m = pick == ns + k
        tgt[m] = lo + g.random((int(m.sum()), 3)) * (hi - lo)
    for k, p in enumerate(spots):
        sl = slice(k * per_spot, (k + 1) * per_spot)
        o_r[sl] = CAM
        tgt[sl] = np.asarray(p) + _unit(g, per_spot) * spot_jitter * g.random((per_spot, 1))
    assert len(spots) * per_spot <= n_r
    fam = [("R", o_r, tgt - o_r)]
    if ns:
        # I
        k = np.arange(n_i) % ns
        rad = np.array([s[0] for s in spheres])[k][:, None]
        cen = np.array([s[1] for s in spheres], dtype=float)[k]
        fam.append(("I", cen + _unit(g, n_i) * rad * 0.95 * g.random((n_i, 1)) ** (1 / 3), _unit(g, n_i)))
        # N: within a degree of the centre (half of them within a tenth of a degree)
        k = np.arange(n_n) % ns
        cen = np.array([s[1] for s in spheres], dtype=float)[k]
        o_n = CAM + (g.random((n_n, 3)) - 0.5) * 0.4
        to = cen - o_n
        to /= np.linalg.norm(to, axis=1, keepdims=True)
        perp = np.cross(to, _unit(g, n_n))
        perp /= np.linalg.norm(perp, axis=1, keepdims=True)
        ang = np.radians(np.where(np.arange(n_n) % 2 == 0, 1.0, 0.1) * g.random(n_n))
        fam.append(("N", o_n, to + np.tan(ang)[:, None] * perp))
    o = np.concatenate([f[1] for f in fam])
    d = np.concatenate([f[2] for f in fam])
    family = np.concatenate([np.full(len(f[1]), f[0]) for f in fam])
    assert len(o) <= 4096
    return o, d, family


# ---- what a ray's events say -----------------------------------------------------------------------------
# Events of one ray: the restatement's TRACE -- ("light", kind, index, node, lt_mult), ("blocked", index, node),
# ("lit", index, node), ("fresnel", full|simple, enter|leave, TIR, tr, node), ("mirror", node, point) -- plus, from
# the wrappers below, ("shade", generation, node, object index, the material has children) for every shaded hit
# and ("sray", node, object index, N.L, N.H, blocked) for every shadow ray cast.
EPS = 1e-7


def ev(events, kind):
    return [e for e in events if e[0] == kind]


def lights(events, index=None, kind=None):
    return [e for e in events if e[0] == "light" and (index is None or e[2] == index) and (kind is None or e[1] == kind)]


def _after_light(events, index, what):
    """The `what` ("lit" / "blocked") events of light `index`."""
    return [e for e in events if e[0] == what and e[1] == index]


def gate(events):
    """A hit on a material that has children, at the generation that gets none."""
    return any(e[1] >= GATE and e[4] for e in ev(events, "shade"))


def fres(events, shader=None, side=None, tir=None, node_min=1, pred=None):
    return [e for e in ev(events, "fresnel") if (shader is None or e[1] == shader) and (side is None or e[2] == side)
            and (tir is None or e[3] == tir) and e[5] >= node_min and (pred is None or pred(e))]


def two_children(e):  # the full shader's thresholds
    return (not e[3]) and e[4] > EPS and (1 - e[4]) > EPS


class Fixture:
    """name, text, rays, whether a specular term lies on any path, the indices the CPU test restates,
    reach: {branch: (predicate over a ray's events, floor)}, siblings: [(what changed, text, branch whose
    rays must move)], prims: {creation index: label} for per-object figures."""

    def __init__(self, name, text, spheres, specular, reach, siblings, seed, check=None, boxes=(), prims=None, rays=None):
        self.name, self.text, self.spheres, self.specular = name, text, spheres, specular
        self.reach, self.siblings, self.prims = reach, siblings, prims or {}
        self.o, self.d, self.family = make_rays(spheres, seed, boxes=boxes, **(rays or {}))
        n = len(self.o)
        self.check = np.arange(n) if check is None else np.arange(0, n, max(1, n // check))  # a stride keeps every family
        assert len(self.check) >= 512 and set(self.family[self.check]) == set(self.family)


# ---- the fixtures ----------------------------------------------------------------------------------------
def _spot_bands():
    spheres = [(0.6, (-0.8, -0.4, -5.0)), (0.5, (1.2, -0.5, -4.5))]
    spot0 = "spotlight 0 4 -5  0 -1 0  10 25  .9 .8 .7"
    head = HEAD + [spot0, "push", "translate 2 1 -1", "spotlight 0 4 -5  -0.3 -1 0.2  18 18  .5 .6 .9", "pop"] + GREY
    body = ["diffuse .8 .3 .3 .1 .1 .1", _sphere(*spheres[0]), "diffuse .3 .8 .3 .1 .1 .1", _sphere(*spheres[1])]
    text = _text(head, body)
    reach = {}
    for li in (0, 1):
        reach["light %d full" % li] = (lambda E, li=li: any(e[4] == 1 for e in lights(E, li)), 32)
        reach["light %d skipped" % li] = (lambda E, li=li: any(e[4] == 0 for e in lights(E, li)), 32)
        reach["light %d lit" % li] = (lambda E, li=li: bool(_after_light(E, li, "lit")), 32)
        reach["light %d blocked" % li] = (lambda E, li=li: bool(_after_light(E, li, "blocked")), 32)
    reach["light 0 band"] = (lambda E: any(0 < e[4] < 1 for e in lights(E, 0)), 32)
    sib = [("spot 0 made a point light", text.replace(spot0, "point_light 0 4 -5 .9 .8 .7"), "light 0 skipped"),
           ("spot 0 made a point light", text.replace(spot0, "point_light 0 4 -5 .9 .8 .7"), "light 0 band")]
    return Fixture("spot_bands", text, spheres, False, reach, sib, 1)


def _light_mix():
    spheres = [(0.7, (-1.2, -0.3, -5.0)), (0.6, (1.3, -0.4, -4.2))]
    spot = "spotlight -3 5 -4  0.4 -1 -0.2  15 40  .3 .25 .2"
    L = ["point_light 3 4 -2 .3 .3 .3", spot, "disk_light 0 5 -6  0.8  0 -1 0  .25 .3 .3", "push", "translate -1 0.5 1",
         "point_light 2 3 -3 .2 .3 .2", "disk_light 1 4 -7  0.6  0.2 -1 0.1  .3 .2 .3", "pop", "point_light 0 -3 -5 .2 .2 .2",
         "point_light -4 1 -8 .15 .15 .2"]
    text = _text(HEAD, L, GREY, "diffuse .8 .5 .3 .1 .1 .1", _sphere(*spheres[0]), "diffuse .3 .5 .8 .1 .1 .1", _sphere(*spheres[1]))
    kinds = ["point", "spot", "disk", "point", "disk", "point", "point"]
    reach = {"%s %d lit" % (k, i): (lambda E, i=i: bool(_after_light(E, i, "lit")), 32) for i, k in enumerate(kinds)}
    reach.update({"%s %d blocked" % (k, i): (lambda E, i=i: bool(_after_light(E, i, "blocked")), 32) for i, k in enumerate(kinds) if i != 5})
    reach["N.L <= 0, shadow ray cast and free"] = (lambda E: any(e[3] <= EPS and not e[5] for e in ev(E, "sray")), 32)
    reach["N.L <= 0, shadow ray cast and blocked"] = (lambda E: any(e[3] <= EPS and e[5] for e in ev(E, "sray")), 32)
    sib = [("the spot made a point light", text.replace(spot, "point_light -3 5 -4 .3 .25 .2"),
            "spot 1 dimmed")]
    reach["spot 1 dimmed"] = (lambda E: any(e[4] < 1 for e in lights(E, 1)), 32)
    return Fixture("light_mix", text, spheres, False, reach, sib, 2)


def _no_lights():
    spheres = [(0.8, (-1.0, -0.2, -5.0)), (0.6, (1.1, -0.4, -4.5))]
    mirror = "reflective .3 .5 .7 .2 .3 .1 0.6"
    text = _text(HEAD, "reflective .5 .5 .5 .15 .1 .05 0.3", FLOOR, mirror, _sphere(*spheres[0]), "diffuse .8 .2 .2 .3 .2 .1", _sphere(*spheres[1]))
    reach = {"mirror child": (lambda E: bool(ev(E, "mirror")) and not ev(E, "light") and not ev(E, "sray"), 32),
             "ambient only": (lambda E: bool(ev(E, "shade")) and not ev(E, "mirror") and not ev(E, "light"), 32)}
    sib = [("krefl 0", text.replace(mirror, "reflective .3 .5 .7 .2 .3 .1 0"), "sphere mirror")]
    reach["sphere mirror"] = (lambda E: any(e[3] == 2 and e[1] < GATE for e in ev(E, "shade")), 32)
    return Fixture("no_lights", text, spheres, False, reach, sib, 3)


PHONG_ROW = (0, 1, 2, 3, 7.25, 0.5, 33, 160, 1023, 1024, 1025, 2000, -2)


def pow_path(e):
    """The path pow_shade takes for exponent e: None (no specular term), 'square' or 'pow_call'."""
    if e == 0:
        return None
    return "square" if (0 <= e <= 1024 and e == math.floor(e)) else "pow_call"


def highlight(r, c, light, eye=CAM):
    """The point of sphere (r, c) whose normal halves the directions to the light and to the eye."""
    p = c + r * (light - c) / np.linalg.norm(light - c)
    for _ in range(8):
        h = (light - p) / np.linalg.norm(light - p) + (eye - p) / np.linalg.norm(eye - p)
        p = c + r * h / np.linalg.norm(h)
    return p


def _phong_row():
    spheres = [(0.4, ((i % 7 - 3) * 1.0 + (0.5 if i >= 7 else 0.0), -0.6, -6.5 + 1.8 * (i // 7))) for i in range(len(PHONG_ROW))]
    mats = ["shiny .5 .4 .3 .1 .1 .1 .9 .8 .7 %r 0" % e for e in PHONG_ROW]
    L = ["point_light 2 4 1 .6 .6 .6", "point_light -3 2 -2 .4 .4 .5"]
    text = _text(HEAD, L, GREY, [x for m, s in zip(mats, spheres) for x in (m, _sphere(*s))])
    lights_at = [np.array([2.0, 4.0, 1.0]), np.array([-3.0, 2.0, -2.0])]
    spots = [highlight(r, np.asarray(c), lp) for r, c in spheres for lp in lights_at]
    reach = {}
    for i, e in enumerate(PHONG_ROW):
        k = i + 2  # the object index: two floor triangles first
        if e == 0:
            reach["exponent 0: lit, no term"] = (lambda E, k=k: any(s[2] == k and not s[5] for s in ev(E, "sray")), 32)
        else:
            reach["exponent %r: hdp > EPS" % e] = (lambda E, k=k: any(s[2] == k and not s[5] and s[4] > EPS for s in ev(E, "sray")), 32)
    reach["hdp <= EPS"] = (lambda E: any(s[2] >= 3 and not s[5] and s[4] <= EPS for s in ev(E, "sray")), 32)
    sib = [("specular colour 0", text.replace(" .9 .8 .7 ", " 0 0 0 "), "exponent %r: hdp > EPS" % e) for e in PHONG_ROW if e]
    return Fixture("phong_row", text, spheres, True, reach, sib, 4, prims={i + 2: e for i, e in enumerate(PHONG_ROW)},
                   rays=dict(n_r=3072, n_i=256, n_n=768, spots=spots))


def _mirrors():
    spheres = [(1.0, (-1.02, 0.1, -5.0)), (1.0, (1.02, 0.1, -5.0))]
    a, b = "reflective .2 .2 .2 .1 .1 .1 0.85", "shiny .1 .1 .3 .05 .05 .1 .6 .6 .6 40 0.9"
    text = _text(HEAD, "point_light 1 5 0 .8 .8 .8", GREY, a, _sphere(*spheres[0]), b, _sphere(*spheres[1]))
    reach = {"mirror child": (lambda E: bool(ev(E, "mirror")), 32),
             "chain to the gate": (gate, 8),
             "reflection off the inside, no child": (lambda E: any(e[1] == 0 and e[3] >= 2 for e in ev(E, "shade")) and not ev(E, "mirror"), 32)}
    sib = [("krefl 0", text.replace(a, "reflective .2 .2 .2 .1 .1 .1 0").replace(b, "shiny .1 .1 .3 .05 .05 .1 .6 .6 .6 40 0"), "mirror child"),
           ("specular colour 0", text.replace(" .6 .6 .6 40", " 0 0 0 40"), "specular on sphere b")]
    reach["specular on sphere b"] = (lambda E: any(s[2] == 3 and not s[5] and s[4] > 0.9 for s in ev(E, "sray")), 32)
    return Fixture("mirrors", text, spheres, True, reach, sib, 5, boxes=[((-0.12, -0.6, -5.7), (0.12, 0.8, -4.3))] * 2)


def _tri_only():
    mat = "shiny .6 .5 .4 .1 .1 .1 .7 .7 .8 12.5 0.4"
    g = np.random.default_rng(6)
    tris = []
    for k in range(9):  # a fan of tilted triangles over the floor, in a BVH (leaf size 5, the root drops one: Q1)
        c = np.array([-2.4 + 0.6 * k, -0.2 + 0.1 * (k % 3), -5.0 - 0.25 * (k % 4)])
        tris.append(np.round((c + g.integers(-40, 41, size=(3, 3)) / 64.0) * 64) / 64)
    bvh = ["begin_list"] + ["%s" % x for t in tris for x in (["begin"] + ["vertex %r %r %r" % tuple(float(q) for q in v) for v in t] + ["end"])] + ["end_accel"]
    wall = ["begin", "vertex -3 -1 -8", "vertex 3 -1 -8", "vertex 0 3 -9", "end"]
    text = _text(HEAD, "point_light 2 5 0 .6 .6 .6", "point_light -3 3 -2 .4 .4 .5", mat, FLOOR, wall, bvh)
    reach = {"mirror child": (lambda E: bool(ev(E, "mirror")), 32),
             "specular, hdp > EPS": (lambda E: any(not s[5] and s[4] > EPS for s in ev(E, "sray")), 32),
             "blocked": (lambda E: bool(ev(E, "blocked")), 32)}
    sib = [("specular colour 0", text.replace(" .7 .7 .8 12.5", " 0 0 0 12.5"), "specular, hdp > EPS"),
           ("krefl 0", text.replace("12.5 0.4", "12.5 0"), "mirror child")]
    return Fixture("tri_only", text, [], True, reach, sib, 6, boxes=[((-3, -1, -8.5), (3, 2.5, -4.5))] * 2)


def _surface(index, perm=0.4, clr=(.9, .7, .5)):
    return "surface .3 .2 .1 .05 .05 .05 0 0 0 0 0 %r %r %r %r %r" % (index, perm, *clr)


def _glass(name, index, seed, other, extra_reach, check=None, rays=None, spheres=((1.0, (0.0, 0.2, -5.0)),), boxes=(), second=None):
    """One `surface` glass of the given index on every sphere; second: the index of every other sphere."""
    spheres = list(spheres)
    mats = [_surface(index), _surface(second, 0.3, (.6, .8, .9)) if second else _surface(index)]
    text = _text(HEAD, "point_light 2 5 0 .8 .8 .8", GREY, [x for k, s in enumerate(spheres) for x in (mats[k % 2], _sphere(*s))])
    reach = {"enter": (lambda E: bool(fres(E, "full", "enter")), 32)}
    reach.update(extra_reach)
    sib = [("index %r -> %r" % (index, other), text.replace(_surface(index), _surface(other)), "enter")]
    return Fixture(name, text, spheres, False, reach, sib, seed, check=check, rays=rays, boxes=boxes)


def _glass_full():
    deep = 2 ** (GATE - 1)  # a node of the last generation that still has children
    return _glass("glass_full", 1.5, 7, 1.4, {
        "leave below the critical angle": (lambda E: bool(fres(E, "full", "leave", False)), 32),
        "total internal reflection": (lambda E: bool(fres(E, "full", "leave", True)), 32),
        "two children": (lambda E: bool(fres(E, "full", pred=two_children)), 32),
        "two children at the deepest level": (lambda E: bool(fres(E, "full", node_min=deep, pred=two_children)), 8),
        "two children at every level": (lambda E: {int(math.log2(e[5])) for e in fres(E, "full", pred=two_children)} >= set(range(GATE)), 8),
        "gate": (gate, 8)}, check=1024, spheres=[(1.0, (0.0, 0.3, z)) for z in (-4.0, -6.1, -8.2, -10.3)], second=1.8)
    # A row seen end-on: two generations a sphere. The indices alternate 1.5 / 1.8 because a ray that has been
    # through glass keeps that glass's medium for good (both children get it, myObjShader.java:248,264), so it
    # enters glass of the same index with n1 == n2, tr == 0 and one child.


def _glass_near_one():
    return _glass("glass_near_one", 1.0004, 8, 1.3, {
        "refraction child only (tr <= EPS)": (lambda E: bool(fres(E, "full", tir=False, pred=lambda e: e[4] <= EPS)), 32),
        "two children": (lambda E: bool(fres(E, "full", pred=two_children)), 32)}, rays=dict(n_r=1024, n_i=1024, n_n=2048))


def _glass_below_one():
    return _glass("glass_below_one", 0.8, 9, 0.9, {
        "every leaving hit is TIR": (lambda E: bool(fres(E, "full", "leave")) and not fres(E, "full", "leave", False), 32),
        "entering past the critical angle (NaN tr: no child)": (lambda E: bool(fres(E, "full", "enter", pred=lambda e: e[4] != e[4])), 32),
        "NaN cos2 under a finite tr: the refraction ray misses everything": (
            lambda E: bool(fres(E, "full", "enter", pred=lambda e: e[5] == 1 and two_children(e))) and not any(e[2] == 2 for e in ev(E, "shade")), 32),
        "entering below it": (lambda E: bool(fres(E, "full", "enter", pred=two_children)) and any(e[2] == 2 for e in ev(E, "shade")), 32)})


SIMPLE = ((0.8, 1.6), (0.8, 1.05), (0, 1.3))


def _glass_simple():
    spheres = [(0.7, (-1.6, -0.2, -5.0)), (0.7, (0.0, -0.2, -4.6)), (0.7, (1.6, -0.2, -5.0))]
    mat = lambda kt, ri: "shiny .3 .3 .4 .1 .1 .1 0 0 0 0 0.5 %r %r" % (kt, ri)  # noqa: E731
    text = _text(HEAD, "point_light 2 5 0 .8 .8 .8", GREY, [x for (kt, ri), s in zip(SIMPLE, spheres) for x in (mat(kt, ri), _sphere(*s))])
    on = lambda E, k: {e[2] for e in ev(E, "shade") if e[3] == k}  # noqa: E731
    reach = {"simple enter": (lambda E: bool(fres(E, "simple", "enter")), 32),
             "simple leave": (lambda E: bool(fres(E, "simple", "leave", False)), 32),
             "simple TIR": (lambda E: bool(fres(E, "simple", "leave", True)), 32),
             "simple, both children": (lambda E: bool(fres(E, "simple", pred=lambda e: e[4] > 0 and 1 - e[4] > 0)), 32),
             "ktrans 0: a mirror under the simple flag": (lambda E: bool(on(E, 4)) and bool(ev(E, "mirror")), 32)}
    for k in (2, 3):
        reach["sphere %d entered" % k] = (lambda E, k=k: bool(on(E, k)) and bool(fres(E, "simple", "enter")), 32)
    sib = [("index 1.6 -> 1.5", text.replace(mat(0.8, 1.6), mat(0.8, 1.5)), "sphere 2 entered"),
           ("index 1.05 -> 1.1", text.replace(mat(0.8, 1.05), mat(0.8, 1.1)), "sphere 3 entered"),
           ("krefl 0", text.replace(mat(0, 1.3), "shiny .3 .3 .4 .1 .1 .1 0 0 0 0 0 0 1.3"), "ktrans 0: a mirror under the simple flag")]
    return Fixture("glass_simple", text, spheres, False, reach, sib, 10)


def _glass_nested():
    ca, cb = (-1.4, 0.3, -5.0), (1.4, 0.3, -5.0)
    spheres = [(1.2, ca), (0.5, ca), (1.2, cb), (0.5, cb)]
    outer, inner, simple = _surface(1.5), _surface(1.2, 0.3, (.6, .9, .7)), "shiny .3 .3 .4 .1 .1 .1 0 0 0 0 0.5 0.8 1.3"
    text = _text(HEAD, "point_light 2 5 0 .8 .8 .8", GREY, outer, _sphere(*spheres[0]), inner, _sphere(*spheres[1]),
                 outer, _sphere(*spheres[2]), simple, _sphere(*spheres[3]))
    # an entering split on a ray that is no camera ray: its n1 is the medium the ray carries
    reach = {"full inside full: n1 from entry 0": (lambda E: bool(fres(E, "full", "enter", node_min=2)) and any(e[3] == 3 for e in ev(E, "shade")), 32),
             "simple inside full: n1 from entry 1": (lambda E: bool(fres(E, "simple", "enter", node_min=2)), 32),
             "NaN cos2 entering the inner sphere": (lambda E: any(e[3] == 3 for e in ev(E, "shade")) and
                                                    bool(fres(E, "full", "enter", node_min=2, pred=lambda e: e[4] != e[4] or e[4] > 0.5)), 8)}
    sib = [("outer index 1.5 -> 1.4", text.replace(outer, _surface(1.4)), "full inside full: n1 from entry 0"),
           ("outer perm 0.4 -> 0.6", text.replace(outer, _surface(1.5, 0.6)), "simple inside full: n1 from entry 1"),
           ("the inner sphere's medium removed", text.replace(inner, "diffuse .6 .9 .7 .05 .05 .05"), "full inside full: n1 from entry 0"),
           ("the inner sphere's medium removed", text.replace(simple, "diffuse .3 .3 .4 .1 .1 .1"), "simple inside full: n1 from entry 1")]
    return Fixture("glass_nested", text, spheres, False, reach, sib, 11)


BUILDERS = {"spot_bands": _spot_bands, "light_mix": _light_mix, "no_lights": _no_lights, "phong_row": _phong_row, "mirrors": _mirrors,
            "tri_only": _tri_only, "glass_full": _glass_full, "glass_near_one": _glass_near_one, "glass_below_one": _glass_below_one,
            "glass_simple": _glass_simple, "glass_nested": _glass_nested}
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return BUILDERS[name]()


def write_all(d):
    """Every fixture's .cli text into directory d."""
    for n in NAMES:
        (d / (n + ".cli")).write_text(fixture(n).text)


# ---- the restatement, ray by ray -------------------------------------------------------------------------
def _planars(sc):
    return [o for obj in sc.objs for o in (obj.members if hasattr(obj, "members") else [obj]) if hasattr(o, "v")]


def _instrument(m, sc):
    """Wrap the scene's shading entries so that TRACE also gets the `shade` and `sray` events."""
    index = {id(o): i for i, o in enumerate(sc.objs)}
    cur = []
    color_at, shadow_color, shadowed = sc.color_at, sc.shadow_color, sc.shadowed

    def color_at_w(h, key):
        m.TRACE.append(("shade", h.trans_ray.gen, h.trans_ray.node, index.get(id(h.obj), -1), h.obj.shader.has_caustic))
        return color_at(h, key)

    def shadow_color_w(h, tex, key):
        cur.append(h)
        try:
            return shadow_color(h, tex, key)
        finally:
            cur.pop()

    def shadowed_w(ray, dist):
        h = cur[-1]
        nl = m.dot(ray.d, h.nrm)
        nh = m.dot(m.normalize(m.sub(ray.d, h.fwd_dir)), h.nrm)
        blocked = shadowed(ray, dist)
        m.TRACE.append(("sray", h.trans_ray.node, index.get(id(h.obj), -1), nl, nh, blocked))
        return blocked

    sc.color_at, sc.shadow_color, sc.shadowed = color_at_w, shadow_color_w, shadowed_w


@functools.lru_cache(maxsize=None)
def restated(name, sample):
    """(colours [len(check), 3], the events of each ray) of fixture `name`'s check rays by the restatement:
    reflectRay of myRay(o, d) under the key {SEED, FIRST_KEY + i, sample, node 1}. Planar objects are put back
    into their never-hit state after each ray (trace_util.load_reference says why)."""
    fx = fixture(name)
    m = tu.make_kats()
    sc = m.load(fx.text, 64, 64)
    _instrument(m, sc)
    flat = _planars(sc)
    cols, events = [], []
    for i in fx.check:
        m.TRACE.clear()
        c = sc.reflect_ray(m.Ray(fx.o[i], fx.d[i], 0), (SEED, FIRST_KEY + int(i), sample))
        cols.append(c)
        events.append(list(m.TRACE))
        for p in flat:
            p._setup()
    m.TRACE.clear()
    return np.asarray(cols, dtype=np.float64), events


def reached(name, branch, sample=0):
    """Boolean mask over the fixture's check rays: the restatement took `branch` on that ray."""
    pred = fixture(name).reach[branch][0]
    return np.array([bool(pred(E)) for E in restated(name, sample)[1]])


def same_or_nan(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def deviation(a, b):
    """max |a - b| with NaN == NaN counted as 0 and NaN against a number as inf."""
    d = np.abs(a - b)
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, np.where(np.isnan(d), np.inf, d))
    return d
