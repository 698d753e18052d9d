"""The upload-time table of the triangles-only kernels (csrc/rt_types.h, trace.hip hit_tables_kernel): a
triangle hit's world normal, read per (triangle, orientation) by make_hit (RT_HIT_NRM), against the
statements it replaces (the all-features kernels never take the table) and against the oracle. The lights
are those a table of light positions would be about (measured and not built): they stay
as cases of the light CTM.

Scene (objList order): two ground triangles under the identity (0, 1); one triangle under its own rotate +
non-uniform scale CTM (2, xfc = -1); a list of 300 random triangles, a zero-area one and a needle under
translate + rotate + non-uniform scale (3); a list of axis-aligned triangles, whose normals have two zero
components, under a scale with one negative factor (4). A reflective `surface`; a point light under the
identity with a zero coordinate and one declared inside push / translate / rotate / scale / pop.

Tolerances are those of tests/test_gpu_prims.py: t and pos bit-equal, the normal to test_gpu_trace.TOL on
rays whose two nearest candidates are further apart than 1e-9 relative (no more than 1 % are not), everything
discrete exact; radiance and frames by tests/parity.py. Default against generic is bit for bit throughout."""
import numpy as np
import pytest

from distraytracer_old_amd import rt
from tests import parity
from tests import trace_util as tu
from tests.test_gpu_shade import _pack
from tests.test_gpu_trace import TOL, _rel, _same_bits

pytestmark = pytest.mark.gpu

SEED = tu.SEED
FIRST_KEY = 1000
BUILDER_BLOCK = 256  # threads per block of hit_tables_kernel (trace.hip HIT_TABLES_BLOCK): one per triangle
MODES = {"packet": 0, "lanes": rt.TRACE_LANES, "sort": rt.TRACE_SORT}
FIELDS = ("flags", "prim", "top", "args", "material", "t", "pos", "normal")
OWN_CENTRE, LIST_CENTRE, AXIS_CENTRE = np.array([2.5, 0.0, -4.0]), np.array([0.25, 0.0, -4.0]), np.array([-2.5, 0.0, -4.0])
OWN_TRI = np.array([[[-1, -0.75, 0], [1, -0.5, 0.25], [0, 1, -0.25]]])
ZERO_AREA = np.array([[[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [0.75, 0.75, 0.75]]])
NEEDLE = np.array([[[-0.75, 0.5, 0.25], [0.75, 0.5, 0.25], [0, 0.515625, 0.25]]])
LIGHTS = ["point_light 3 4 0 .8 .8 .8",
          "push", "translate -2.5 3 -1.5", "rotate 30 0 1 0", "scale 1 2 0.5", "point_light 0.25 0.5 0 .5 .5 .6", "pop"]


def axis_tris(n=96, seed=SEED + 7):
    """n triangles, each in a plane x / y / z = const (grid 1/64): normals with two zero components."""
    g = np.random.default_rng(seed)
    t = g.integers(-40, 41, size=(n, 1, 3)) + g.integers(-30, 31, size=(n, 3, 3))
    for k in range(n):
        t[k, :, k % 3] = t[k, 0, k % 3]
    return t / 64.0


def scene_text():
    L = ["fov 60", "background 0.1 0.1 0.2", *LIGHTS, "surface .8 .8 .8 .2 .2 .2 .5 .5 .5 20 0.3"]
    L += tu._tri_lines(tu.GROUND, 1.0)
    L += ["push", "translate %r %r %r" % tuple(OWN_CENTRE.tolist()), "rotate 40 1 0 1", "scale 1.5 0.5 1"]
    L += tu._tri_lines(OWN_TRI, 1.0) + ["pop"]
    L += ["surface .7 .5 .3 .1 .1 .1 .4 .4 .4 12 0.25", "push", "translate %r %r %r" % tuple(LIST_CENTRE.tolist()), "rotate 35 1 2 0.5",
          "scale 1.25 0.75 1.5", "begin_list"]
    L += tu._tri_lines(np.concatenate([tu.random_tris(300, SEED + 5), ZERO_AREA, NEEDLE]), 1.0)
    L += ["end_accel", "pop", "push", "translate %r %r %r" % tuple(AXIS_CENTRE.tolist()), "scale 1 -1.25 0.75", "begin_list"]
    L += tu._tri_lines(axis_tris(), 1.0)
    L += ["end_accel", "pop"]
    return "\n".join(L) + "\n"


N_TRI = 2 + 1 + 302 + 96


def build_rays():
    """16,384 rays: towards points in each object's region from every side, so both faces of its triangles are
    met; the ground from above and from below."""
    g = np.random.default_rng(SEED + 8)
    parts = []
    for centre, half, n in ((LIST_CENTRE, 0.9, 6144), (AXIS_CENTRE, 0.8, 6144), (OWN_CENTRE, 0.4, 2048)):
        target = centre + (g.random((n, 3)) * 2 - 1) * half
        u = g.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        parts.append((target - u * (3.0 + 3.0 * g.random((n, 1))), u))
    n = 2048
    target = np.stack([g.random(n) * 12 - 6, np.full(n, -1.5), g.random(n) * 12 - 10], 1)
    u = g.normal(size=(n, 3))
    u[:, 1] = np.where(np.arange(n) % 2 == 0, -1, 1) * (0.2 + np.abs(u[:, 1]))  # even: from above, odd: from below
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    parts.append((target - u * (2.0 + 2.0 * g.random((n, 1))), u))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


class Case:
    def __init__(self, d):
        from oracle.oracle import OracleScene

        self.dir_path = d
        (d / "gen_tables.cli").write_text(scene_text())
        self.o = OracleScene(d, "gen_tables.cli", {})
        self.g = rt.Scene.load_cli("gen_tables.cli", scene_dir=d, textures={})
        self.origin, self.dir = build_rays()
        self.ref = self.o.trace(self.origin, self.dir, seed=SEED, first_key=FIRST_KEY)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    c = Case(tmp_path_factory.mktemp("hit_tables"))
    yield c
    c.g.close()
    c.o.close()


def test_the_scene_and_rays_are_what_the_test_is_about(case):
    """The triangles-only kernels run (variant F = 0), and each orientation wins at least 1,000 records, at least
    100 in each list, and some on the ground and on the triangle with its own CTM."""
    assert case.g.variant() == (0, 0)
    info = case.g.info()
    assert info["objects"] == case.o.info()["objects"] == 5 and info["triangles"] == N_TRI and info["lights"] == 2
    ref = case.ref
    assert len(case.origin) == 16384
    hit = ref["hit"]
    for side in (0, 1):
        m = hit & (ref["args"] == side)
        per_top = np.bincount(ref["top"][m], minlength=5)
        print("orientation", side, "records", int(m.sum()), "per objList entry", per_top.tolist())
        assert m.sum() >= 1000 and per_top[3] >= 100 and per_top[4] >= 100 and per_top[2] >= 100 and per_top[:2].sum() >= 100
    assert (ref["in_accel"][hit] == (ref["top"][hit] >= 3)).all()


def test_records_default_against_generic(case):
    """make_hit<0> reads the table; the all-features instantiation runs the two normalisations and the adjoint
    product. Every field of every record is the same bits, in the packet, per-lane and sorted modes."""
    o, d = case.origin, case.dir
    failures = []
    for mode, fl in MODES.items():
        want = case.g.trace(o, d, seed=SEED, first_key=FIRST_KEY, flags=fl | rt.TRACE_GENERIC)
        got = case.g.trace(o, d, seed=SEED, first_key=FIRST_KEY, flags=fl)
        diff = _same_bits(got, want, fields=FIELDS)
        if diff:
            failures.append((mode, diff))
        assert ((want["flags"] & rt.HIT_HIT) != 0).sum() >= 2000
    assert not failures, failures


def test_records_match_the_oracle(case):
    ref, o, d = case.ref, case.origin, case.dir
    hit, wide = ref["hit"], ref["gap"] > 1e-9
    left_out = int((hit & ~wide).sum())
    print("records left out by the gap rule", left_out, "of", len(o))
    assert max(TOL.values()) <= 1e-9 and left_out <= 0.01 * len(o)
    failures = []
    for mode, fl in MODES.items():
        h = case.g.trace(o, d, seed=SEED, first_key=FIRST_KEY, flags=fl)
        got_hit = (h["flags"] & rt.HIT_HIT) != 0
        checks = {"bad": ((h["flags"] & rt.HIT_BAD_RAY) != 0) != ref["bad"], "hit": got_hit != hit, "prim": h["prim"] != ref["prim"],
                  "top": h["top"] != ref["top"], "args": (h["args"] != ref["args"]) & hit,
                  "in-accel flag": ((h["flags"] & rt.HIT_IN_ACCEL) != 0) != ref["in_accel"]}
        for what, bad in checks.items():
            if bad.any():
                failures.append((mode, what, int(bad.sum()), np.flatnonzero(bad)[:6].tolist()))
        for f in ("t", "pos", "normal"):
            m = hit & got_hit & wide
            r = _rel(h[f][m], ref[f][m])
            r = r if r.ndim == 1 else r.max(1)
            worst = float(r.max()) if not np.isnan(r).any() else float("nan")
            print(mode, f, "worst", worst, "differing", int((r > 0).sum()))
            if not worst <= TOL[f]:
                failures.append((mode, f, worst, int((~(r <= TOL[f])).sum())))
    assert not failures, failures


def test_radiance_default_against_generic_and_the_oracle(case):
    o, d = case.origin, case.dir
    got, gst = case.g.shade(o, d, seed=SEED, first_key=FIRST_KEY, sample=0, flags=0)
    gen, nst = case.g.shade(o, d, seed=SEED, first_key=FIRST_KEY, sample=0, flags=rt.TRACE_GENERIC)
    assert np.array_equal(gst, nst) and np.array_equal(got.view(np.uint8), gen.view(np.uint8))
    want, wst = case.o.shade(o, d, seed=SEED, first_key=FIRST_KEY, sample=0)
    assert np.array_equal(gst, wst)
    cmp = parity.compare(got[:, None, :], _pack(got)[:, None], want[:, None, :], _pack(want)[:, None])
    print(cmp, "colours", len(np.unique(_pack(want))))
    parity.assert_exact_decisions(cmp)
    assert len(np.unique(_pack(want))) > 20


def test_frame_default_against_generic_wavefront_and_the_oracle(case):
    rg, ag = case.g.render(64, 64, spp=4, seed=SEED)
    for flags in (rt.RENDER_GENERIC, rt.RENDER_WAVEFRONT):
        rb, ab = case.g.render(64, 64, spp=4, seed=SEED, flags=flags)
        assert np.array_equal(ag, ab), flags
        assert np.array_equal(rg.view(np.uint32), rb.view(np.uint32)), flags
    ro, ao, _ = case.o.render(64, 64, spp=4, seed=SEED)
    cmp = parity.compare(rg, ag, ro, ao)
    print(cmp, "colours", len(np.unique(ao)))
    parity.assert_exact_decisions(cmp)
    assert len(np.unique(ao)) > 50


# ---- sizes around the builder kernel's block, light counts, tables per scene -------------------------------
GRID_SHIFT, GRID_SCALE = np.array([0.0, 0.0, -6.0]), np.array([1.0, 1.0, 2.0])
MORE_LIGHTS = ["push", "rotate 20 1 0 0", "point_light 0 5 2 .3 .3 .3", "pop"]


def grid_tris(n):
    """n disjoint triangles about the plane z = 0, 20 to a row, each inside its own 1/4 cell and tilted by its
    own amount (the reference's box test misses a list whose box has no extent along an axis)."""
    i = np.arange(n)
    c = np.stack([(i % 20 - 9.5) / 4, (i // 20 - 6) / 4, np.zeros(n)], 1)
    off = np.array([[-6, -5, 0], [6, -5, 0], [0, 6, 0]]) / 64.0
    t = c[:, None, :] + off[None]
    t[:, 2, 2] = (i % 4 + 1) * np.where(i % 2 == 0, -1, 1) / 64.0
    return t


def grid_text(n, lights):
    L = ["fov 60", "background 0.1 0.1 0.2", *(LIGHTS if lights > 1 else LIGHTS[:1]), *(MORE_LIGHTS if lights > 2 else []),
         "surface .7 .5 .3 .1 .1 .1 .4 .4 .4 12 0.25"]
    if n:
        L += ["push", "translate %r %r %r" % tuple(GRID_SHIFT.tolist()), "scale %r %r %r" % tuple(GRID_SCALE.tolist()), "begin_list"] + tu._tri_lines(grid_tris(n), 1.0) + ["end_list", "pop"]
    return "\n".join(L) + "\n"


def _load_grid(d, n, lights):
    name = f"grid_{n}_{lights}.cli"
    (d / name).write_text(grid_text(n, lights))
    return rt.Scene.load_cli(name, scene_dir=d, textures={})


@pytest.mark.parametrize("n,lights", [(0, 1), (1, 1), (BUILDER_BLOCK - 1, 1), (BUILDER_BLOCK, 3), (BUILDER_BLOCK + 1, 1), (1, 3)])
def test_sizes_around_the_builder_block(n, lights, tmp_path):
    """Triangle counts 0 (background only), 1 and around hit_tables_kernel's block of 256 threads, one and three
    lights (more lights than triangles too): every triangle is met from both sides by a ray aimed at its
    centroid, its record and its radiance are the generic kernel's bits, and so is a small frame."""
    with _load_grid(tmp_path, n, lights) as s:
        assert s.variant() == (0, 0) and s.info()["triangles"] == n and s.info()["lights"] == lights
        ra, aa = s.render(32, 32, spp=2, seed=SEED)
        rb, ab = s.render(32, 32, spp=2, seed=SEED, flags=rt.RENDER_GENERIC)
        assert np.array_equal(aa, ab) and np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
        if n == 0:
            assert len(np.unique(aa)) == 1
            return
        c = grid_tris(n).mean(1) * GRID_SCALE + GRID_SHIFT
        o = np.concatenate([c + [0.125, 0.0625, 3.0], c - [0.125, 0.0625, 3.0]])
        d = np.concatenate([c, c]) - o
        got = s.trace(o, d, seed=SEED, first_key=FIRST_KEY)
        want = s.trace(o, d, seed=SEED, first_key=FIRST_KEY, flags=rt.TRACE_GENERIC)
        assert not _same_bits(got, want, fields=FIELDS)
        assert ((got["flags"] & rt.HIT_HIT) != 0).all() and np.array_equal(got["prim"], np.tile(np.arange(n), 2))
        assert (got["args"][:n] != got["args"][n:]).all() and np.array_equal(got["normal"][:n], -got["normal"][n:])
        sa, _ = s.shade(o, d, seed=SEED, first_key=FIRST_KEY, sample=0)
        sb, _ = s.shade(o, d, seed=SEED, first_key=FIRST_KEY, sample=0, flags=rt.TRACE_GENERIC)
        assert np.array_equal(sa.view(np.uint8), sb.view(np.uint8))


@pytest.mark.parametrize("close_first", ["other", "own"])
def test_tables_are_per_scene(close_first, case, tmp_path):
    """A scene's tables live in its own allocations: loading, rendering and closing another scene with other
    triangle and light counts leaves a scene's frame as it was, whichever of the two is closed first."""
    a = rt.Scene.load_cli("gen_tables.cli", scene_dir=case.dir_path, textures={})
    ra, aa = a.render(64, 64, spp=1, seed=SEED)
    b = _load_grid(tmp_path, BUILDER_BLOCK + 1, 3)
    rb, ab = b.render(64, 64, spp=1, seed=SEED)
    assert not np.array_equal(aa, ab)
    first, second, want = (b, a, (ra, aa)) if close_first == "other" else (a, b, (rb, ab))
    r1, a1 = second.render(64, 64, spp=1, seed=SEED)
    first.close()
    r2, a2 = second.render(64, 64, spp=1, seed=SEED)
    second.close()
    for r, g in ((r1, a1), (r2, a2)):
        assert np.array_equal(g, want[1]) and np.array_equal(r.view(np.uint32), want[0].view(np.uint32))
