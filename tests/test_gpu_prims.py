"""Every primitive type's ray-query record, occlusion and radiance against the oracle's entries for caller
rays (OracleScene.trace / .occluded / .shade, pinned on the CPU by tests/test_oracle_rays.py).

Scenes (tests/trace_util.py): gen_prims -- plane, box, ellipsoid, hollow cylinder, both cylinder forms, glass
sphere, moving sphere, sphereIn, a list of sphere / quad / cyl / triangle under their own CTMs, a named
sphere instanced with and without `shdr`; gen_inst -- a named BVH instanced three times (the two-level
case), an instanced cyl and quad, a list holding an instance, a sierpinski; gen_prims_photon -- gen_prims
under a disk light with a small photon map (radiance only).

Ray families, about 4 k rays per scene under keys {SEED, FIRST_KEY + i}: R random, B bounce rays starting
exactly on the oracle's hit positions, I rays starting inside the closed primitives, X the rejection table;
T rays tangent to every sphere, ellipsoid and cylinder side (through each primitive's or instance's CTM) and
P rays grazing the plane and the box faces are compared between traversal modes only.

Tolerances. t and pos are held to bit equality and the normal to test_gpu_trace.TOL["normal"] (one
re-normalisation of a list member's planar normal), for every primitive type; only
rays whose two smallest candidate t differ by more than 1e-9 relative are compared under a tolerance, and
the others (asserted below 1 %) still go through the mode-to-mode comparison."""
import numpy as np
import pytest

from distraytracer_old_amd import rt
from tests import parity
from tests import trace_util as tu
from tests.test_gpu_shade import _pack
from tests.test_gpu_trace import MODES, REF, TOL, _rel, _same_bits

pytestmark = pytest.mark.gpu

SEED = tu.SEED
FIRST_KEY = 1000
ALL_MODES = {**MODES, "generic": rt.TRACE_GENERIC, "sort": rt.TRACE_SORT}
PHOTON_LINE = "diffuse_photons  20000  50 0.1"
N_MODE = 1 << 14  # rays per family of the mode-to-mode comparison (needs no oracle)

# gen_inst: objList entries (file order) and what reaches a hit through them
INST_TOPS = ["ground", "ground", "BVH instance", "BVH instance", "BVH instance shdr", "cyl instance", "quad instance",
             "list with an instance", "sierpinski"]


class Case:
    """One scene on both sides with its rays and the oracle's records, computed once for the module."""

    def __init__(self, d, name):
        from oracle.oracle import OracleScene

        self.name, self.dir_path = name, d
        self.o = OracleScene(d, f"{name}.cli", {})
        self.g = rt.Scene.load_cli(f"{name}.cli", scene_dir=d, textures={})
        tr = lambda o, dd: self.o.trace(o, dd, seed=SEED, first_key=FIRST_KEY)  # noqa: E731
        ro, rd = tu.shell_rays(2048)
        r = tr(ro, rd)  # R leads the batch: its keys here are its keys there
        bo, bd, _ = tu.bounce_rays(ro, rd, r)
        fam = [("R", ro, rd), ("B", bo, bd)]
        if name != "gen_inst":
            io, idir, self.inside_prim = tu.inside_rays(tr, ro, rd, r, tu.GEN_PRIMS_CLOSED)
            fam.append(("I", io, idir))
        xo, xd, _ = tu.spoil(ro[:300], rd[:300])
        fam.append(("X", xo, xd))
        self.origin = np.concatenate([f[1] for f in fam])
        self.dir = np.concatenate([f[2] for f in fam])
        self.family = np.concatenate([np.full(len(f[1]), f[0]) for f in fam])
        self.ref = tr(self.origin, self.dir)
        assert all(np.array_equal(self.ref[f][:2048], r[f], equal_nan=True) for f in ("t", "prim", "pos"))
        self.r_first = r

    def close(self):
        self.g.close()
        self.o.close()


@pytest.fixture(scope="module")
def case_of(tmp_path_factory):
    d = tmp_path_factory.mktemp("prim_scenes")
    (d / "gen_prims.cli").write_text(tu.gen_prims_text())
    (d / "gen_inst.cli").write_text(tu.gen_inst_text())
    disk = tu.gen_prims_text(disk_light=True)
    assert "spotlight" in disk
    (d / "gen_prims_photon.cli").write_text(disk.replace("spotlight", PHOTON_LINE + "\nspotlight", 1))
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(d, name)
        return cache[name]

    yield get
    for c in cache.values():
        c.close()


def _where(c, bad):
    i = np.flatnonzero(bad)[:6]
    return [(int(k), str(c.family[k]), int(c.ref["prim"][k]), int(c.ref["top"][k])) for k in i]


# ---- conditions on the oracle's output: a degenerate input fails loudly -------------------------------
def test_gen_prims_covers_every_primitive(case_of):
    c = case_of("gen_prims")
    for info in (c.g.info(), rt.inspect_cli("gen_prims.cli", scene_dir=c.dir_path, textures={})):
        assert info["objects"] == c.o.info()["objects"] == 12 and info["prims"] == c.o.info()["prims"] == 14
    ref, fam = c.ref, c.family
    for f, lo, hi in (("R", 0.05, 0.95), ("B", 0.05, 1.0), ("I", 0.05, 1.0)):
        share = ref["hit"][fam == f].mean()
        print("gen_prims", f, int((fam == f).sum()), "rays, hit share", share)
        assert lo <= share <= hi, (f, share)
    hit = ref["hit"] & (fam != "X") & (ref["gap"] > 1e-9)  # the records compared: R, B and I past the gap condition
    count = np.bincount(ref["prim"][hit], minlength=14)
    print("winners per primitive", dict(zip(tu.GEN_PRIMS_TYPES, count.tolist())))
    inside = np.bincount(c.inside_prim, minlength=14)
    assert (inside[list(tu.GEN_PRIMS_CLOSED)] >= 8).all(), inside  # family I starts inside every closed primitive
    assert (count >= 20).all(), count
    for p, want in tu.GEN_PRIMS_ARGS.items():
        assert set(ref["args"][hit & (ref["prim"] == p)].tolist()) == want, tu.GEN_PRIMS_TYPES[p]
    assert (ref["in_accel"][hit] == (ref["top"][hit] == 9)).all() and (ref["instance"][hit] == (ref["top"][hit] >= 10)).all()
    assert min((hit & (ref["top"] == t)).sum() for t in (9, 10, 11)) >= 20


def test_gen_inst_covers_both_instance_kinds(case_of):
    c = case_of("gen_inst")
    assert c.g.info()["objects"] == c.o.info()["objects"] == len(INST_TOPS) and c.g.info()["prims"] == c.o.info()["prims"]
    ref, fam = c.ref, c.family
    for f, lo, hi in (("R", 0.05, 0.95), ("B", 0.05, 1.0)):
        share = ref["hit"][fam == f].mean()
        assert lo <= share <= hi, (f, share)
    hit = ref["hit"] & (fam != "X") & (ref["gap"] > 1e-9)  # the records compared
    count = np.bincount(ref["top"][hit], minlength=len(INST_TOPS))
    print("winners per objList entry", dict(zip(INST_TOPS, count.tolist())))
    assert (count >= 20).all(), count
    # instance of a primitive; instance of an accel or instance held by a list (next line tells them apart);
    # plain list member; plain top-level primitive
    for inst, acc in ((True, False), (True, True), (False, True), (False, False)):
        assert (hit & (ref["instance"] == inst) & (ref["in_accel"] == acc)).sum() >= 20, (inst, acc)
    assert (hit & ref["instance"] & (ref["top"] == 7)).sum() >= 20  # the instance held by the list


# ---- records ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gen_prims", "gen_inst"])
def test_records_match_the_oracle(name, case_of):
    c = case_of(name)
    ref, o, d = c.ref, c.origin, c.dir
    hit = ref["hit"]
    compared = c.family != "X"
    wide = ref["gap"] > 1e-9  # best and second-best candidate apart: a tolerance cannot hide a wrong primitive
    tight = int((hit & compared & ~wide).sum())
    print(name, "rays", len(o), "hits", int(hit.sum()), "rays failing the gap condition", tight)
    assert max(TOL.values()) <= 1e-9 and tight < 0.01 * compared.sum()
    types = tu.GEN_PRIMS_TYPES if name == "gen_prims" else None
    failures = []
    for mode, fl in ALL_MODES.items():
        h = c.g.trace(o, d, seed=SEED, first_key=FIRST_KEY, flags=fl)
        got_hit = (h["flags"] & rt.HIT_HIT) != 0
        checks = {
            "bad": ((h["flags"] & rt.HIT_BAD_RAY) != 0) != ref["bad"],
            "hit": got_hit != hit,
            "prim": h["prim"] != ref["prim"],
            "top": h["top"] != ref["top"],
            "args": (h["args"] != ref["args"]) & hit,
            "instance flag": ((h["flags"] & rt.HIT_INSTANCE) != 0) != ref["instance"],
            "in-accel flag": ((h["flags"] & rt.HIT_IN_ACCEL) != 0) != ref["in_accel"],
            "miss record": ~hit & ~(np.isposinf(h["t"]) & (h["pos"] == 0).all(1) & (h["normal"] == 0).all(1) &
                                    (h["material"] == -1) & (h["args"] == 0)),
        }
        for what, bad in checks.items():
            if bad.any():
                failures.append((mode, what, int(bad.sum()), _where(c, bad)))
        # the material: equal device indices <-> equal oracle fingerprints (every material of the generated
        # scenes has its own diffuse colour), so an instance with `shdr` reports its own, one without the base's
        ok = hit & got_hit
        _, fp_id = np.unique(ref["fp"][ok], axis=0, return_inverse=True)
        pairs = np.unique(np.stack([h["material"][ok], fp_id.ravel()], 1), axis=0)
        if len(np.unique(pairs[:, 0])) != len(pairs) or len(np.unique(pairs[:, 1])) != len(pairs) or (pairs[:, 0] < 0).any():
            failures.append((mode, "material", pairs.tolist()))
        for f in ("t", "pos", "normal"):
            m = ok & wide
            r = _rel(h[f][m], ref[f][m])
            r = r if r.ndim == 1 else r.max(1)
            worst = float(r.max()) if not np.isnan(r).any() else float("nan")
            if types:
                per = {types[p]: float(r[ref["prim"][m] == p].max()) for p in range(len(types)) if (ref["prim"][m] == p).any()}
            else:
                per = {INST_TOPS[t] + f" ({t})": float(r[ref["top"][m] == t].max()) for t in np.unique(ref["top"][m])}
            print(name, mode, f, "worst", worst, "differing", int((r > 0).sum()), {k: v for k, v in per.items() if v > 0})
            if not worst <= TOL[f]:  # a NaN fails
                bad = np.zeros(len(o), bool)
                bad[np.flatnonzero(m)[~(r <= TOL[f])]] = True
                failures.append((mode, f, worst, int(bad.sum()), _where(c, bad)))
    assert not failures, failures


def test_instance_held_by_a_list_reports_both_flags(case_of):
    """An instance that is a member of a list (the list of gen_inst, every sierpinski element) is reached
    through a myInstance and is a list member whose hit reCalcCTMHitNorm rebuilds: RT_HIT_INSTANCE and
    RT_HIT_IN_ACCEL. The query kernel used to report the second only for members tested as plain primitives."""
    c = case_of("gen_inst")
    held = c.ref["hit"] & c.ref["instance"] & np.isin(c.ref["top"], (7, 8))
    assert (held & (c.ref["top"] == 7)).sum() >= 20 and (held & (c.ref["top"] == 8)).sum() >= 20
    assert c.ref["in_accel"][held].all()
    for mode, fl in ALL_MODES.items():
        h = c.g.trace(c.origin[held], c.dir[held], seed=SEED, first_key=FIRST_KEY, flags=fl)
        assert (h["flags"] == (rt.HIT_HIT | rt.HIT_INSTANCE | rt.HIT_IN_ACCEL)).all(), (mode, np.unique(h["flags"]))


@pytest.mark.parametrize("name", ["gen_prims", "gen_inst"])
def test_occlusion_matches_the_oracle(name, case_of):
    c = case_of(name)
    o, d = c.origin, c.dir
    # family B also with tmax = the exact t of its next hit: calcShadow's dist - t > 1e-7 at its edge
    edge = np.where((c.family == "B") & c.ref["hit"], c.ref["t"], np.inf)
    failures = []
    for tmax in (*tu.TMAX, edge):
        want = c.o.occluded(o, d, tmax, seed=SEED, first_key=FIRST_KEY)
        label = "edge" if tmax is edge else tmax
        share = (want[c.family != "X"] == 1).mean()
        print(name, "tmax", label, "occluded share", share)
        # both outcomes occur (at tmax 3 only the bounce rays, which start on a surface, have anything that near)
        assert min((want == 1).sum(), (want == 0).sum()) >= 100, (label, share)
        assert (want[c.family == "X"] == 2).sum() == len(tu.BAD_RAYS)
        for mode, fl in ALL_MODES.items():
            got = c.g.occluded(o, d, tmax, seed=SEED, first_key=FIRST_KEY, flags=fl)
            if not np.array_equal(got, want):
                failures.append((label, mode, int((got != want).sum()), _where(c, got != want)))
    assert not failures, failures


# ---- between modes: T, P and everything else, bit for bit ---------------------------------------------
def _tangent_rays(c, n, seed):
    """Family T: rays tangent to every sphere, ellipsoid and cylinder side of the scene, built in object
    space and taken to world space by each primitive's CTM or its instance's (tu.quadrics: rotated and
    scaled cylinders, instanced and sierpinski spheres, list members), every origin coordinate then moved by
    0 to +-4 ulps; gen_prims' moving sphere by bisection under each ray's own key, in the batch's first
    slots. Discriminants near zero.
    The construction is held to conditions on the oracle's output: with the origins moved 1e-6 along the
    normal into the surface most rays (>= 50 %) of a top-level quadric win on one primitive, moved 1e-6 out
    of it under a tenth of that do. A list tests its members only for rays that pass its own box, which
    the Q4 double transform places elsewhere, so a list's members are held to 20 such rays together."""
    g = np.random.default_rng(seed)
    qs = tu.quadrics((c.dir_path / f"{c.name}.cli").read_text())
    assert len(qs) == (10 if c.name == "gen_prims" else 8)
    os_, ds = [], []
    if c.name == "gen_prims":
        tr = lambda o, d: c.o.trace(o, d, seed=SEED, first_key=FIRST_KEY)  # noqa: E731
        o, d, ok = tu.moving_sphere_tangents(tr, tu.GEN_PRIMS_TYPES.index("moving_sphere"), (-1.5, 1.5, -5), (-1.0, 1.75, -5), 1024, g)
        assert ok.mean() >= 0.9, ok.mean()
        os_.append(o)
        ds.append(d)
    per = (n - sum(len(o) for o in os_)) // len(qs)
    listed = 0
    for q in qs:
        keys = []
        for shift in (-1e-6, 1e-6):
            o, d, _ = tu.tangent_rays(q, 400, np.random.default_rng(seed + 1), shift)
            r = c.o.trace(o, d, seed=SEED, first_key=FIRST_KEY)
            keys.append(np.where(r["hit"], r["prim"] * 1000 + r["top"], -1))
        straddle = keys[0] != keys[1]
        target = np.bincount(keys[0][straddle] + 1).argmax() - 1 if straddle.any() else -2
        cut, passed = (keys[0] == target).mean(), (keys[1] == target).mean()
        print(c.name, "T", q["name"], "listed" if q["listed"] else "top level", "cut", cut, "passed by", passed)
        if q["listed"]:
            listed += int((keys[0] == target).sum()) if passed <= 0.1 * cut else 0
        else:
            assert cut >= 0.5 and passed <= 0.1 * cut, (q["name"], cut, passed)
        o, d, _ = tu.tangent_rays(q, per, g)
        os_.append(tu._nudge(o, g.integers(-4, 5, size=o.shape)))
        ds.append(d)
    assert listed >= 20, listed
    return np.concatenate(os_), np.concatenate(ds)


def _grazing_rays(c, n, seed):
    """Family P over gen_prims: directions within 1e-9 of parallel to the plane and to each face of the
    rotated box (a point and the normal of every face come from the oracle's own records), starting within
    1e-6 of the face's plane; plus exactly axis-aligned directions with signed zeros through the box."""
    g = np.random.default_rng(seed)
    ref = c.ref
    faces = []
    for prim, arg in [(0, 0)] + [(1, a) for a in range(6)]:
        i = np.flatnonzero(ref["hit"] & (ref["prim"] == prim) & (ref["args"] == arg))[0]
        faces.append((ref["pos"][i], ref["normal"][i]))
    k = g.integers(0, len(faces), n)
    p = np.stack([faces[j][0] for j in k])
    nr = np.stack([faces[j][1] for j in k])
    w = np.cross(nr, g.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    d = w + nr * (g.random((n, 1)) * 2e-9 - 1e-9)
    o = p + nr * (g.random((n, 1)) * 2e-6 - 1e-6) - w * (0.5 + 3.0 * g.random((n, 1)))
    # axis-aligned, signed zeros, through the box around (-2, 0, -6)
    m = n // 4
    axis = g.integers(0, 3, m)
    da = np.where(g.random((m, 3)) < 0.5, 0.0, -0.0)
    sign = g.choice([-1.0, 1.0], m)
    da[np.arange(m), axis] = sign
    oa = np.array([-2.0, 0.0, -6.0]) + (g.random((m, 3)) - 0.5) * 1.6
    oa[np.arange(m), axis] -= sign * 3.0
    o[:m], d[:m] = oa, da
    return o, d


def _modes_equal(g, o, d, tmax, what):
    want = g.trace(o, d, seed=SEED, first_key=FIRST_KEY, flags=REF)
    want_occ = g.occluded(o, d, tmax, seed=SEED, first_key=FIRST_KEY, flags=REF)
    share = float(((want["flags"] & rt.HIT_HIT) != 0).mean())
    print(what, len(o), "rays, closest-hit share", round(share, 4), "occluded share", round(float((want_occ == 1).mean()), 4))
    failures = []
    for mode, fl in ALL_MODES.items():
        if fl == REF:
            continue
        got = g.trace(o, d, seed=SEED, first_key=FIRST_KEY, flags=fl)
        diff = _same_bits(got, want, fields=("flags", "prim", "top", "args", "material", "t", "pos", "normal"))
        if diff:
            failures.append((what, mode, diff))
        got_occ = g.occluded(o, d, tmax, seed=SEED, first_key=FIRST_KEY, flags=fl)
        if not np.array_equal(got_occ, want_occ):
            failures.append((what, mode, "occlusion", int((got_occ != want_occ).sum()), np.flatnonzero(got_occ != want_occ)[:8].tolist()))
    return share, failures


@pytest.mark.parametrize("name", ["gen_prims", "gen_inst"])
def test_modes_agree_bit_for_bit(name, case_of):
    """Every traversal mode against the reference's own order (lanes + nocull, fp64 throughout), on every
    family, no tolerance and no exclusions."""
    c = case_of(name)
    rng = np.random.default_rng(9)
    fams = {"RBIX": (c.origin, c.dir)}
    big = tu.shell_rays(N_MODE, seed=SEED + 1)
    fams["R large"] = big
    fams["T"] = _tangent_rays(c, N_MODE, SEED + 2)  # first: the moving sphere's rays keep the slots they were bisected in
    if name == "gen_prims":
        fams["P"] = _grazing_rays(c, N_MODE, SEED + 3)
    failures = []
    for what, (o, d) in fams.items():
        tmax = np.where(rng.random(len(o)) < 0.5, np.inf, 8.0)
        share, f = _modes_equal(c.g, o, d, tmax, f"{name} {what}")
        failures += f
        assert 0.05 <= share <= 0.95, (what, share)
    assert not failures, failures


def test_axis_aligned_box_modes_agree():
    """p3_t04's axis-aligned box: exactly axis-aligned directions with signed zeros, and directions within 1e-9
    of parallel to its faces from origins within 1e-6 of the face planes."""
    g = np.random.default_rng(SEED + 4)
    n = N_MODE
    lo, hi = np.array([-1.0, -1.0, -6.0]), np.array([1.0, 1.0, -4.0])
    axis = g.integers(0, 3, n)
    sign = g.choice([-1.0, 1.0], n)
    d = np.where(g.random((n, 3)) < 0.5, 0.0, -0.0)
    d[np.arange(n), axis] = sign
    o = lo - 0.25 + g.random((n, 3)) * (hi - lo + 0.5)
    o[np.arange(n), axis] = np.where(sign > 0, lo[axis] - 1 - g.random(n), hi[axis] + 1 + g.random(n))
    # second half: grazing a face (component `face` nearly 0, origin on that face's plane +- 1e-6)
    h = n // 2
    face = g.integers(0, 3, h)
    dg = g.normal(size=(h, 3))
    dg[np.arange(h), face] = g.random(h) * 2e-9 - 1e-9
    og = lo + g.random((h, 3)) * (hi - lo) - dg * 3.0
    og[np.arange(h), face] = np.where(g.random(h) < 0.5, lo[face], hi[face]) + g.random(h) * 2e-6 - 1e-6
    o[h:], d[h:] = og, dg
    with rt.Scene.load_cli("p3_t04.cli") as s:
        share, failures = _modes_equal(s, o, d, np.full(n, np.inf), "p3_t04")
    assert 0.05 <= share <= 0.95, share
    assert not failures, failures


# ---- radiance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gen_prims", "gen_inst", "gen_prims_photon"])
def test_radiance_matches_the_oracle(name, case_of):
    """rt_shade_rays on rays that are no camera rays -- bounce rays leaving a surface, rays starting inside glass
    and inside the box, rays from behind a quad -- against reflectRay under the same keys, by the rule every
    deterministic-decision frame is held to (tests/parity.py): per-channel TOL, then exact decisions."""
    c = case_of(name)
    if name == "gen_prims_photon":  # both sides gather over the same photon_list
        c.g.build_photons(SEED)
        pos, pwr = c.g.photons()
        assert len(pos) > 1000
        c.o.set_photons(pos, pwr)
    o, d = c.origin, c.dir
    bad = c.family == "X"
    for sample in (0, 3):
        want, wst = c.o.shade(o, d, seed=SEED, first_key=FIRST_KEY, sample=sample)
        for mode, fl in (("packet", 0), ("sort", rt.TRACE_SORT)):
            got, gst = c.g.shade(o, d, seed=SEED, first_key=FIRST_KEY, sample=sample, flags=fl)
            assert np.array_equal(gst, wst) and (gst[bad] == 2).sum() == len(tu.BAD_RAYS)
            cmp = parity.compare(got[:, None, :], _pack(got)[:, None], want[:, None, :], _pack(want)[:, None])
            worst = np.abs(got - want).max(1)
            print(name, "sample", sample, mode, cmp, "colours", len(np.unique(_pack(want))), _where(c, worst > parity.TOL))
            parity.assert_exact_decisions(cmp)
        assert len(np.unique(_pack(want))) > 20
