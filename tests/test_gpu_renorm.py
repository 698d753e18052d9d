"""The compiled kernels on rays chosen by how their direction behaves under repeated normalisation
(csrc/trace_device.h renorm / unit_len, make_hit's direction reuse, the light distance, planar_test's sign
test): ray-query records, occlusion, radiance and a rendered frame against the oracle.

Scene: two ground triangles at the top level in front of a list of 300 triangles under a translate + rotate +
non-uniform scale CTM, two point lights, a reflective `surface`. Rays (15,360 = 240 waves of 64), picked on the
host with the classifier of tests/test_renorm_identity.py, each aimed at the list's region:
  fixed    whole waves whose directions are fixed by the ray constructor's normalisation,
  one_osc  such waves carrying exactly one period-2 direction, its lane moving from wave to wave,
  mixed    directions fixed after 1, 2 and 3 normalisations and period-2 ones, interleaved,
  scaled   the same kind of mixture from directions of length 3.7 (un-normalised input),
  axis     axis-aligned directions with signed zeros (48 waves of them, each direction many times).
Tolerances are those of tests/test_gpu_prims.py: t and pos bit-equal, the normal to test_gpu_trace.TOL (the
reference's second in-place normalisation of a list member's stored N), on rays whose two
nearest candidates are further apart than 1e-9 relative; everything discrete exact; radiance and the frame by
tests/parity.py."""
import numpy as np
import pytest

from distraytracer_old_amd import rt
from tests import parity
from tests import trace_util as tu
from tests.test_gpu_shade import _pack
from tests.test_gpu_trace import TOL, _rel
from tests.test_renorm_identity import _nrmz, classify

pytestmark = pytest.mark.gpu

SEED = tu.SEED
FIRST_KEY = 1000
WAVES = 48  # per family
MODES = {"packet": 0, "lanes": rt.TRACE_LANES}
CENTRE = np.array([0.25, 0.0, -4.0])


def scene_text():
    L = ["fov 60", "background 0.1 0.1 0.2", "point_light 3 4 0 .8 .8 .8", "point_light -2.5 3 -1.5 .5 .5 .6",
         "surface .8 .8 .8 .2 .2 .2 .5 .5 .5 20 0.3"]
    L += tu._tri_lines(tu.GROUND, 1.0)
    L += ["surface .7 .5 .3 .1 .1 .1 .4 .4 .4 12 0.25", "push", "translate 0.25 0 -4", "rotate 35 1 2 0.5", "scale 1.25 0.75 1.5",
          "begin_list"]
    L += tu._tri_lines(tu.random_tris(300, SEED + 5), 1.0)
    L += ["end_accel", "pop"]
    return "\n".join(L) + "\n"


def _axis_dirs(n, g):
    d = np.where(g.random((n, 3)) < 0.5, 0.0, -0.0)
    d[np.arange(n), g.integers(0, 3, n)] = g.choice([-1.0, 1.0], n)
    return d


def _mixed(pool, n):
    m = np.empty((n, 3))
    for j, k in enumerate((0, 1, 2, -2)):
        m[j::4] = np.resize(pool[k], (n // 4, 3))
    return m


def build_rays():
    """Classes are those of the direction the ray constructor makes of the input (nrmz(d)): 0, 1, 2 further
    normalisations until it is fixed, -2 a period-2 cycle."""
    g = np.random.default_rng(SEED + 6)
    u = _nrmz(g.normal(size=(250_000, 3)))[0]
    cu = classify(u, steps=8)
    cu = np.where(cu > 0, cu - 1, cu)  # the constructor's normalisation is the first of u's
    pool = {k: u[cu == k] for k in (0, 1, 2, -2)}
    s = u[:120_000] * 3.7
    cs = classify(_nrmz(s)[0], steps=8)
    spool = {k: s[cs == k] for k in (0, 1, 2, -2)}
    n = WAVES * 64
    sizes = {k: (len(pool[k]), len(spool[k])) for k in pool}
    assert len(pool[0]) >= 3 * n and len(pool[1]) >= n // 4 and min(sizes[2]) >= 300 and min(sizes[-2]) >= 500, sizes
    fixed = pool[0][:n]
    one = pool[0][n:2 * n].copy()
    lanes = (np.arange(WAVES) * 7 + 3) % 64
    one[np.arange(WAVES) * 64 + lanes] = pool[-2][:WAVES]
    pool[0], pool[-2] = pool[0][2 * n:], pool[-2][WAVES:]
    mixed, scaled = _mixed(pool, n), _mixed(spool, n)
    fam = {"fixed": fixed, "one_osc": one, "mixed": mixed, "scaled": scaled, "axis": _axis_dirs(n, g)}
    d = np.concatenate(list(fam.values()))
    family = np.concatenate([np.full(n, k) for k in fam])
    unit = _nrmz(d)[0]
    target = CENTRE + (g.random((len(d), 3)) - 0.5) * np.array([2.5, 1.5, 2.5])
    o = target - unit * (3.0 + 3.0 * g.random((len(d), 1)))
    return o, d, family, lanes


class Case:
    def __init__(self, d):
        from oracle.oracle import OracleScene

        (d / "gen_renorm.cli").write_text(scene_text())
        self.o = OracleScene(d, "gen_renorm.cli", {})
        self.g = rt.Scene.load_cli("gen_renorm.cli", scene_dir=d, textures={})
        self.origin, self.dir, self.family, self.lanes = build_rays()
        self.ref = self.o.trace(self.origin, self.dir, seed=SEED, first_key=FIRST_KEY)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    c = Case(tmp_path_factory.mktemp("renorm_scene"))
    yield c
    c.g.close()
    c.o.close()


def test_the_rays_are_what_the_test_is_about(case):
    """Conditions on the input: 16,384 rays at the most, whole waves of fixed directions, waves with exactly one
    period-2 lane, and every family hitting both the top-level triangles and the list's members."""
    o, d, fam = case.origin, case.dir, case.family
    assert len(o) == 5 * WAVES * 64 <= 16384 and case.g.info()["objects"] == case.o.info()["objects"] == 3
    cls = classify(_nrmz(d)[0], steps=8).reshape(-1, 64)
    wf = fam.reshape(-1, 64)[:, 0]
    assert (cls[wf == "fixed"] == 0).all()
    one = cls[wf == "one_osc"]
    assert ((one == -2).sum(1) == 1).all() and ((one == 0).sum(1) == 63).all()
    assert np.array_equal(np.argmax(one == -2, 1), case.lanes) and len(np.unique(case.lanes)) >= 32
    for f in ("mixed", "scaled"):
        c = cls[wf == f]
        assert all(((c == k).sum(1) == 16).all() for k in (0, 1, 2, -2)), f
    ref = case.ref
    for f in np.unique(fam):
        m = fam == f
        top = ref["hit"][m] & ~ref["in_accel"][m]
        acc = ref["hit"][m] & ref["in_accel"][m]
        print(f, "rays", int(m.sum()), "top-level hits", int(top.sum()), "list hits", int(acc.sum()), "misses", int((~ref["hit"][m]).sum()))
        assert top.sum() >= 200 and acc.sum() >= 200, f
    both = np.bincount(ref["args"][ref["hit"]], minlength=2)
    assert both.min() >= 500, both  # triangles hit from the front and from the back


def test_records_match_the_oracle(case):
    ref, o, d = case.ref, case.origin, case.dir
    hit, wide = ref["hit"], ref["gap"] > 1e-9
    assert (hit & ~wide).sum() < 0.01 * len(o)
    failures = []
    for mode, fl in MODES.items():
        h = case.g.trace(o, d, seed=SEED, first_key=FIRST_KEY, flags=fl)
        got_hit = (h["flags"] & rt.HIT_HIT) != 0
        checks = {"bad": ((h["flags"] & rt.HIT_BAD_RAY) != 0) != ref["bad"], "hit": got_hit != hit, "prim": h["prim"] != ref["prim"],
                  "top": h["top"] != ref["top"], "args": (h["args"] != ref["args"]) & hit,
                  "in-accel flag": ((h["flags"] & rt.HIT_IN_ACCEL) != 0) != ref["in_accel"]}
        for what, bad in checks.items():
            if bad.any():
                failures.append((mode, what, int(bad.sum()), np.flatnonzero(bad)[:6].tolist(), case.family[bad][:6].tolist()))
        for f in ("t", "pos", "normal"):
            m = hit & got_hit & wide
            r = _rel(h[f][m], ref[f][m])
            r = r if r.ndim == 1 else r.max(1)
            worst = float(r.max()) if not np.isnan(r).any() else float("nan")
            print(mode, f, "worst", worst, "differing", int((r > 0).sum()))
            if not worst <= TOL[f]:
                failures.append((mode, f, worst, int((~(r <= TOL[f])).sum())))
    assert not failures, failures


def test_occlusion_matches_the_oracle(case):
    o, d = case.origin, case.dir
    failures = []
    for tmax in tu.TMAX:
        want = case.o.occluded(o, d, tmax, seed=SEED, first_key=FIRST_KEY)
        print("tmax", tmax, "occluded share", (want == 1).mean())
        assert min((want == 1).sum(), (want == 0).sum()) >= 100, tmax
        for mode, fl in MODES.items():
            got = case.g.occluded(o, d, tmax, seed=SEED, first_key=FIRST_KEY, flags=fl)
            if not np.array_equal(got, want):
                failures.append((tmax, mode, int((got != want).sum()), case.family[got != want][:6].tolist()))
    assert not failures, failures


def test_radiance_matches_the_oracle(case):
    o, d = case.origin, case.dir
    want, wst = case.o.shade(o, d, seed=SEED, first_key=FIRST_KEY, sample=0)
    got, gst = case.g.shade(o, d, seed=SEED, first_key=FIRST_KEY, sample=0, flags=0)
    assert np.array_equal(gst, wst)
    cmp = parity.compare(got[:, None, :], _pack(got)[:, None], want[:, None, :], _pack(want)[:, None])
    print(cmp, "colours", len(np.unique(_pack(want))))
    parity.assert_exact_decisions(cmp)
    assert len(np.unique(_pack(want))) > 20


def test_frame_matches_the_oracle(case):
    """64 x 64 at 16 spp through the render kernel's own packet path: no decision mismatch, ARGB exact."""
    rg, ag = case.g.render(64, 64, spp=16, seed=SEED)
    ro, ao, _ = case.o.render(64, 64, spp=16, seed=SEED)
    cmp = parity.compare(rg, ag, ro, ao)
    print(cmp, "colours", len(np.unique(ao)))
    parity.assert_exact_decisions(cmp)
    assert np.array_equal(ag, ao)
    assert len(np.unique(ao)) > 50
