"""Shared by tests/test_knn_space.py (CPU) and tests/test_gpu_knn_space.py (GPU): the photon gather
(irradiance<> in csrc/trace_kernels.h) against brute force over the branches its answer goes through.

Three kinds of things live here, and they are kept apart on purpose:

* the EXPECTED VALUES: brute_force (a stable sort of every photon's find_near distance) and the
  oracle's find_near (oracle_reference). Nothing else is ever the expected value of a gather.
* an INDEPENDENT RESTATEMENT of the photon BVH (numpy_photon_map), written from the description at the
  top of csrc/photon.cpp: sort-based, no code shared with either builder.
* a MODEL OF THE KERNEL'S CONTROL FLOW (start_window, bracket_model, wave_lanewise). It says which
  branches a query takes -- the start window, the widen exits, the histogram widths, the narrow edge
  walk, the level cap, shell overflow, the lane-wise scan -- and is used only to prove that a fixture
  reaches the branch it is named for (the reach floors of tests/test_knn_space.py).

Plain numpy; nothing here needs a GPU."""
import functools
import math
import tempfile
from pathlib import Path

import numpy as np

PI_F = 3.1415927410125732  # (double)PConstants.PI
PI_D = 3.141592653589793   # Math.PI
PHOTON_LEAF = 24           # photons per leaf of the photon BVH
KNN_START = 1.15           # RT_KNN_START
KNN_SHELL = 10             # RT_KNN_SHELL
KNN_HB = 128               # buckets of a counting pass
KNN_LEVELS = 32
DIV_R, DIV_FRAC = 2.0, 2   # RT_KNN_DIV_R, RT_KNN_DIV_FRAC


# ---------------------------------------------------------------------------------------------
# scenes
def scene_text(k, max_dist):
    """The smallest scene with a diffuse photon map of neighbourhood k within max_dist."""
    return (f"fov 60\nbackground 0 0 0\npoint_light 0 5 0 1 1 1\ndiffuse_photons 100 {k} {max_dist!r}\n"
            "diffuse .5 .5 .5 0 0 0\nsphere 1 0 0 -5\n")


def plane_scene_text(k, max_dist):
    """A photon-mapped quad at z = -4 that fills a 60 degree view from the origin."""
    return (f"fov 60\nbackground 0 0 0\npoint_light 0 3 0 1 1 1\ndiffuse_photons 100 {k} {max_dist!r}\n"
            "diffuse .6 .6 .6 .1 .1 .1\nbegin quad\nvertex -3 -3 -4\nvertex 3 -3 -4\nvertex 3 3 -4\nvertex -3 3 -4\nend\n")


def max_dist2(max_dist):
    """max_dist^2 as both loaders form it: the text goes through Float.parseFloat."""
    md = float(np.float32(max_dist))
    return md * md


# ---------------------------------------------------------------------------------------------
# expected values
def find_near_d2(pos, q):
    """myKD_Tree.find_near's len2 of every photon: dx*dx + dy*dy + dz*dz, in that order."""
    dx, dy, dz = q[0] - pos[:, 0], q[1] - pos[:, 1], q[2] - pos[:, 2]
    return dx * dx + dy * dy + dz * dz


def brute_force(pos, pwr, q, k, max_dist):
    """(irradiance [3], photon indices of the set nearest first, straddle): the k nearest photons with
    d2 < max_dist^2 by a stable sort, their powers summed exactly (math.fsum) over PI_F * (k-th d2).
    straddle: the (k+1)-th kept distance equals the k-th -- only the reference's kd-tree order and
    heap decide which of them is in the set."""
    d2 = find_near_d2(pos, q)
    kept = np.flatnonzero(d2 < max_dist2(max_dist))
    kept = kept[np.argsort(d2[kept], kind="stable")]
    sel = kept[:k]
    if len(sel) == 0:
        return np.zeros(3), sel, False
    straddle = len(kept) > k and d2[kept[k]] == d2[kept[k - 1]]
    s = np.array([math.fsum(pwr[sel, c]) for c in range(3)])
    with np.errstate(divide="ignore", invalid="ignore"):
        return s / np.float64(PI_F * d2[sel[-1]]), sel, bool(straddle)


def oracle_irradiance(o, pwr, q):
    """getIrradianceFromPhtnTree over the oracle's find_near: (irradiance, indices, d2) with the powers
    summed in poll order (farthest first) over PI_F * d2[0]."""
    idx, d2 = o.knn(q)
    if len(idx) == 0:
        return np.zeros(3), idx, d2
    s = np.zeros(3)
    for i in idx:
        s = s + pwr[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        return s / np.float64(PI_F * d2[0]), idx, d2


@functools.lru_cache(maxsize=None)
def oracle_reference(name, k, max_dist):
    """The oracle's answer to every query of a fixture, computed once per process and shared:
    (irradiance [nq, 3], straddle [nq], the photon indices of each set in poll order). Read-only."""
    from oracle.oracle import OracleScene

    fx = fixture(name)
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "knn.cli").write_text(scene_text(k, max_dist))
        o = OracleScene(d, "knn.cli")
        o.set_photons(fx["pos"], fx["pwr"])
        irr = np.zeros((len(fx["q"]), 3))
        straddle = np.zeros(len(fx["q"]), dtype=bool)
        sets = []
        for j, q in enumerate(fx["q"]):
            irr[j], idx, d2 = oracle_irradiance(o, fx["pwr"], q)
            idx.setflags(write=False)
            sets.append(idx)
            if len(idx) == k:
                all_d2 = find_near_d2(fx["pos"], q)
                straddle[j] = int((all_d2 == d2[0]).sum()) > int((d2 == d2[0]).sum())
        o.close()
    for a in (irr, straddle):
        a.setflags(write=False)
    return irr, straddle, tuple(sets)


# ---------------------------------------------------------------------------------------------
# the photon BVH, restated
def numpy_photon_map(pos, pwr=None):
    """The photon map of a photon list in Scene.photon_map()'s form: (nodes uint8 [n_nodes, 128], root,
    leaf-ordered positions, leaf-ordered powers).

    A range of photons is split at lo + cnt // 2 on the axis of largest extent (a later axis only on
    a strictly greater extent); its left half is the smallest photons by (coordinate + 0.0, index).
    A range of <= 24 photons is a leaf, its photons in index order -- except the root, always a node:
    a map of <= 24 photons is one leaf and an empty one with the box (1e300, -1e300). Nodes are
    numbered in DFS pre-order; a node records, per side, the child's box, its node index (-1: a leaf)
    and its range (first, count), the subtree's photon count in padR[1], and the root the number of
    nodes in padR[2] (where the reference's kd-tree follows them)."""
    from distraytracer_old_amd.rt import NODE_DTYPE

    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    pwr = np.zeros((n, 3)) if pwr is None else np.ascontiguousarray(pwr, dtype=np.float64)
    order = np.arange(n)
    recs = []

    def box(a, b):
        if b == a:
            return np.full(3, 1e300), np.full(3, -1e300)
        p = pos[order[a:b]]
        return p.min(0), p.max(0)

    def child(a, b):
        if b - a > PHOTON_LEAF:
            return node(a, b)
        order[a:b] = np.sort(order[a:b])
        return -1

    def node(lo, hi):
        me = len(recs)
        recs.append(None)
        mid = hi
        if hi - lo > PHOTON_LEAF:
            ix = order[lo:hi].copy()
            ext = pos[ix].max(0) - pos[ix].min(0)
            ax = 0
            for c in (1, 2):
                if ext[c] > ext[ax]:
                    ax = c
            order[lo:hi] = ix[np.lexsort((ix, pos[ix, ax] + 0.0))]
            mid = lo + (hi - lo) // 2
        (lmin, lmax), (rmin, rmax) = box(lo, mid), box(mid, hi)  # (a child reorders only within its range)
        left = child(lo, mid)
        right = child(mid, hi)
        recs[me] = (lmin, lmax, left, (lo, mid - lo, mid), rmin, rmax, right, (hi - mid, hi - lo, 0))
        return me

    if n == 0:
        return np.zeros((0, 128), np.uint8), 0, pos.copy(), pwr.copy()
    node(0, n)
    nodes = np.zeros(len(recs), dtype=NODE_DTYPE)
    for i, r in enumerate(recs):
        for f, v in zip(("lmin", "lmax", "left", "pad", "rmin", "rmax", "right", "padR"), r):
            nodes[f][i] = v
    nodes["padR"][0, 2] = len(recs)
    return nodes.view(np.uint8).reshape(len(recs), 128), 0, pos[order].copy(), pwr[order].copy()


def as_nodes(raw):
    """photon_map()'s raw node bytes as a NODE_DTYPE array."""
    from distraytracer_old_amd.rt import NODE_DTYPE

    return np.ascontiguousarray(raw).view(NODE_DTYPE).ravel()


# ---------------------------------------------------------------------------------------------
# the kernel's control flow, restated (reach only -- never an expected value)
def _box_d2(mn, mx, p):
    d = [(p[c] - mn[c]) if p[c] < mn[c] else ((p[c] - mx[c]) if p[c] > mx[c] else 0.0) for c in range(3)]
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]


def start_node(nodes, root, p, K):
    """The node irradiance<> takes its start window from: from the root, into the first internal
    child that holds >= K photons and contains p, until there is none."""
    N = root
    while True:
        nd = nodes[N]
        nxt = -1
        for ref, cnt, mn, mx in ((nd["left"], nd["pad"][1], nd["lmin"], nd["lmax"]),
                                 (nd["right"], nd["padR"][0], nd["rmin"], nd["rmax"])):
            if ref >= 0 and cnt >= K and nxt < 0 and _box_d2(mn, mx, p) == 0.0:
                nxt = int(ref)
        if nxt < 0:
            return N
        N = nxt


def start_window(nodes, root, p, K, R2max):
    """(R2dens, R2far) as irradiance<> computes them: R2far the squared distance to the start node's
    far corner x (1 + 2^-40), R2dens the d^2 holding KNN_START x K photons at the node's density over
    its two largest extents; both capped by R2max, and R2max where the node holds fewer than K."""
    p = [float(x) for x in p]
    nd = nodes[start_node(nodes, root, p, K)]
    if nd["padR"][1] < K:
        return R2max, R2max
    mn = np.minimum(nd["lmin"], nd["rmin"])
    mx = np.maximum(nd["lmax"], nd["rmax"])
    e = [float(mx[c] - mn[c]) for c in range(3)]
    f = [max(p[c] - float(mn[c]), float(mx[c]) - p[c]) for c in range(3)]
    far2 = (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]
    R2far = min(R2max, far2 * (1 + 2.0 ** -40))
    a = max(max(e[0] * e[1], e[0] * e[2]), e[1] * e[2])
    R2dens = min(R2far, KNN_START * K * a / (PI_D * float(nd["padR"][1])))
    return R2dens, R2far


def bracket_model(d2_sorted, K, R2dens, R2far, R2max, u16max=65535):
    """The events one query goes through in irradiance<>'s bracket loop, given every photon's d2 in
    ascending order. Booleans: widen_ext / widen_far / widen_max (the start window held fewer than K
    photons and was widened to the density extrapolation / the node's far corner / max_dist^2), all
    (fewer than K photons within max_dist), u16 / u32 (a counting pass repeated on the same grid
    through u16 / u32 counters), narrow (a pass over a window 2^30 times narrower than hi: the edge
    walk), levels_out (32 levels without bracketing), collapsed (the window emptied), shell_overflow (more window
    photons than the sorted shell holds), replay (the lane replays find_near), on_edge (a photon's d2
    equal to a bucket edge in a pass that takes the one-compare bucket index). Count: passes (levels
    run, as R_KNN_NPASS counts them)."""
    d = np.asarray(d2_sorted, dtype=np.float64)
    ev = dict.fromkeys(("widen_ext", "widen_far", "widen_max", "all", "u16", "u32", "narrow", "levels_out",
                        "collapsed", "shell_overflow", "replay", "on_edge"), False)
    ev["passes"] = 0
    lo, hi, below = 0.0, float(R2dens), 0

    def counts(tot):  # bucket j = #{edges e[k] = lo + (k + 1) w <= d2, k < 127} of the 128-bucket grid
        w = (hi - lo) * (1.0 / KNN_HB)
        edges = lo + np.arange(1, KNN_HB, dtype=np.float64) * w
        if (hi - lo) > hi * 2.0 ** -30 and np.isin(d[:tot], edges).any():
            ev["on_edge"] = True
        return np.bincount(np.searchsorted(edges, d[:tot], side="right"), minlength=KNN_HB)

    for _ in range(KNN_LEVELS):
        ev["passes"] += 1
        tot = int(np.searchsorted(d, hi, side="left"))
        if not ((hi - lo) > hi * 2.0 ** -30):
            ev["narrow"] = True
        c = counts(tot)
        cum = np.cumsum(c)
        if tot > u16max or c.max() > 255:  # the same grid again through wider counters, a part at a time
            ev["u16"] = True
            ev["u32"] = tot > u16max or ev["u32"]
        if tot < K:
            if hi == R2max:
                ev["all"] = True
                break
            ext = hi * (KNN_START * K / float(tot)) if tot > 0 else R2far
            lo, below = hi, tot
            if hi < R2far:
                ev["widen_ext" if ext < R2far else "widen_far"] = True
                hi = min(R2far, ext)
            else:
                ev["widen_max"] = True
                hi = R2max
            continue
        kb = int(np.argmax(cum >= K))
        wp = (hi - lo) * (1.0 / KNN_HB)
        nhi = hi if kb == KNN_HB - 1 else lo + (kb + 1) * wp
        nlo = lo + kb * wp if kb else lo
        below = int(cum[kb - 1]) if kb else below
        lo, hi = nlo, nhi
        if int(cum[kb]) - below <= KNN_SHELL or not (lo < hi):
            ev["collapsed"] = not (lo < hi) and int(cum[kb]) - below > KNN_SHELL
            break
    else:
        ev["levels_out"] = True
    if not ev["all"]:
        i0, i1 = int(np.searchsorted(d, lo, side="left")), int(np.searchsorted(d, hi, side="left"))
        m, need = i1 - i0, K - below
        ev["shell_overflow"] = m > KNN_SHELL
        ev["replay"] = need >= 1 and (m > KNN_SHELL or (need < m and d[i0 + need - 1] == d[i0 + need]))
    return ev


def wave_lanewise(points, R2dens_of_first):
    """The `lw` rule for the <= 64 points of one gather call: at least two lanes, and at least half of
    them, farther than DIV_R start radii of the first lane from the first lane's point."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    d2 = find_near_d2(p, p[0])
    nfar = int((~(d2 <= (DIV_R * DIV_R) * R2dens_of_first)).sum())
    return nfar >= 2 and DIV_FRAC * nfar >= len(p)


def model_events(name, k, max_dist, u16max=65535):
    """bracket_model of every query of a fixture over the numpy photon map (the GPU test holds both
    product builders to that map)."""
    fx = fixture(name)
    raw, root = photon_map_of(name)[:2]
    nodes = as_nodes(raw)
    R2max = max_dist2(max_dist)
    out = []
    for q in fx["q"]:
        R2dens, R2far = start_window(nodes, root, q, k, R2max)
        out.append(bracket_model(np.sort(find_near_d2(fx["pos"], q)), k, R2dens, R2far, R2max, u16max))
    return out


@functools.lru_cache(maxsize=None)
def photon_map_of(name):
    fx = fixture(name)
    return numpy_photon_map(fx["pos"], fx["pwr"])


# ---------------------------------------------------------------------------------------------
# fixtures: fixed seeds, positions shuffled after construction
def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _ball(rng, n, r):
    return _unit(rng, n) * (r * rng.random((n, 1)) ** (1.0 / 3.0))


def _plane(scale):
    rng = np.random.default_rng(101)
    pos = np.concatenate([rng.uniform(-3, 3, size=(5000, 2)), np.full((5000, 1), -4.0)], 1)
    q = np.concatenate([rng.uniform(-3.5, 3.5, size=(256, 2)), -4.0 + rng.normal(0, 0.01, size=(256, 1))], 1)
    return pos * scale, q * scale, rng


def _fixture(name):
    if name in ("plane", "plane_small", "plane_large"):
        s = {"plane": 1.0, "plane_small": 1e-4, "plane_large": 1e5}[name]
        pos, q, rng = _plane(s)
    elif name == "cluster":  # a clump 2000 times denser in radius than its surroundings
        rng = np.random.default_rng(102)
        pos = np.concatenate([_ball(rng, 4000, 1e-3), rng.uniform(-2, 2, size=(1000, 3))])
        q = np.concatenate([rng.normal(0, 1e-3, size=(64, 3)), rng.uniform(-2, 2, size=(128, 3)),
                            rng.normal(0, 0.05, size=(64, 3))])
    elif name == "shell":  # 300 distinct distances within 6e-11 of d2 = 1
        rng = np.random.default_rng(103)
        far = _unit(rng, 60) * (2.0 + rng.random((60, 1)))
        pos = np.concatenate([_unit(rng, 300) * (1.0 + np.arange(300)[:, None] * 1e-13), far])
        q = np.concatenate([np.zeros((1, 3)), rng.normal(0, 1e-13, size=(63, 3))])
    elif name == "big":  # more photons below one window than the u16 buckets count
        rng = np.random.default_rng(104)
        corners = np.array([(x, y, z) for x in (-1., 1.) for y in (-1., 1.) for z in (-1., 1.)])
        pos = np.concatenate([rng.normal(0, 1e-3, size=(70000, 3)), corners])
        q = np.concatenate([rng.normal(0, 1e-3, size=(32, 3)), rng.uniform(-1, 1, size=(32, 3))])
    elif name == "dup":
        # the repeated point lies beyond the others on x, so the 40 copies are one BVH node of zero
        # extent: the query on it starts from a far corner at distance 0 and a window [0, 0)
        rng = np.random.default_rng(105)
        pt = np.array([1.25, 0.1, -0.2])
        pos = np.concatenate([np.tile(pt, (40, 1)), rng.uniform(-1, 1, size=(40, 3))])
        q = np.concatenate([rng.uniform(-1, 1, size=(63, 3)), pt[None]])
    elif name == "edges":
        # d2 exactly ON the first pass's bucket edges: a half-offset 32 x 32 lattice of spacing 2^-4 in
        # the plane z = 0 and queries on x = 0 between its columns. The root splits on x there, so no
        # child box holds a query and the window starts from the root: eight far corners make its
        # density estimate and far corner exceed max_dist^2 = 2^-2, the window is [0, 2^-2) with
        # edges at multiples of 2^-9, and every d2 = ((2i+1)^2 + (2j+1)^2) 2^-10 is (4t + 1) 2^-9.
        rng = np.random.default_rng(107)
        h = 2.0 ** -4
        ij = (np.stack(np.meshgrid(np.arange(-16, 16), np.arange(-16, 16), indexing="ij"), -1).reshape(-1, 2) + 0.5) * h
        corners = np.array([(x, y, z) for x in (-64., 64.) for y in (-64., 64.) for z in (-64., 64.)])
        pos = np.concatenate([np.concatenate([ij, np.zeros((len(ij), 1))], 1), corners])
        q = np.stack([np.zeros(16), np.arange(-8, 8) * h, np.zeros(16)], 1)
    elif name.startswith("few"):
        n = int(name[3:])
        rng = np.random.default_rng(106 + n)
        pos = rng.uniform(-1, 1, size=(n, 3))
        q = rng.uniform(-1.5, 1.5, size=(64, 3))
    else:
        raise KeyError(name)
    pos = pos[rng.permutation(len(pos))]
    pwr = rng.random((len(pos), 3)) * 0.01
    return pos, pwr, q


@functools.lru_cache(maxsize=None)
def fixture(name):
    """{"pos", "pwr", "q", "params": [(k, max_dist), ...]} of a named fixture (read-only arrays)."""
    pos, pwr, q = _fixture(name)
    for a in (pos, pwr, q):
        a.setflags(write=False)
    return {"pos": pos, "pwr": pwr, "q": q, "params": PARAMS[name]}


FEW = ("few1", "few24", "few25", "few30")
FIXTURES = ("plane", "plane_small", "plane_large", "cluster", "shell", "big", "dup", "edges") + FEW
PARAMS = {
    "plane": [(1, .5), (10, .5), (50, .5), (256, .5), (50, .05)],
    "plane_small": [(50, .5 * 1e-4)], "plane_large": [(50, .5 * 1e5)],
    "cluster": [(1, 10.), (50, 10.), (256, 10.), (50, .3)],
    "shell": [(12, 100.), (100, 100.), (256, 100.)],
    "big": [(50, 10.), (256, 10.)],
    "dup": [(20, 100.), (1, 100.)],
    "edges": [(4, .5), (10, .5), (12, .5), (50, .5), (100, .5)],
    "few1": [(50, 100.), (50, .5), (1, 100.), (2, 100.)],
    "few24": [(50, 100.), (50, .5), (24, 100.), (25, 100.), (23, 100.)],
    "few25": [(50, 100.), (50, .5), (25, 100.), (26, 100.), (24, 100.)],
    "few30": [(50, 100.), (50, .5), (30, 100.), (31, 100.), (29, 100.)],
}
CASES = [(name, k, md) for name in FIXTURES for (k, md) in PARAMS[name]]
CASE_IDS = [f"{name}-k{k}-r{md:g}" for name, k, md in CASES]


def plane_render_photons():
    """Photons for plane_scene_text's quad: the plane fixture's layout, a 1,500-photon clump of radius
    1e-3 and one point repeated 40 times, all in the quad's plane and inside the view."""
    pos, _, rng = _plane(1.0)
    a = rng.uniform(0, 2 * np.pi, size=1500)
    r = 1e-3 * np.sqrt(rng.random(1500))
    clump = np.stack([0.52 + r * np.cos(a), 0.31 + r * np.sin(a), np.full(1500, -4.0)], 1)
    dup = np.tile(np.array([-0.83, -0.58, -4.0]), (40, 1))
    pos = np.concatenate([pos, clump, dup])
    pos = pos[rng.permutation(len(pos))]
    return pos, rng.random((len(pos), 3)) * 0.01
