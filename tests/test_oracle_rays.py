"""The oracle's entries for caller rays (OracleScene.trace / .occluded / .shade), pinned on the CPU before
any GPU test relies on them.

1. Records against the plain-Python restatement (tests/golden/make_kats.py through trace_util) on gen_a
   and gen_b: two independent restatements of findClosestRayHit / calcShadow vouch for the entry.
2. Shade against the oracle's own render: camera rays under the frame's keys reproduce a 1-spp frame.
3. Order independence: a batch traced reversed gives the same records.
4. The rejection table of test_gpu_trace.py, through the oracle entry.
5. The generated all-primitives scene is not degenerate: counts, hit shares, every primitive and every
   face argument occur (the conditions test_gpu_prims.py asserts again on the rays it compares)."""
import math

import numpy as np
import pytest

from distraytracer_old_amd import scenes
from oracle.oracle import OracleScene
from tests import trace_util as tu
from tests.test_gpu_trace import TOL

NORMAL_TOL = TOL["normal"]  # one re-normalisation
RECORD_FIELDS = ("hit", "instance", "in_accel", "bad", "prim", "top", "args", "t", "pos", "normal", "fp", "gap")


@pytest.fixture(scope="module")
def gen_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("oracle_rays")
    (d / "gen_a.cli").write_text(tu.scene_text("a"))
    (d / "gen_b.cli").write_text(tu.scene_text("b"))
    (d / "gen_prims.cli").write_text(tu.gen_prims_text())
    return d


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, fields=RECORD_FIELDS):
    return [f for f in fields if not np.array_equal(_bits(a[f]), _bits(b[f]))]


@pytest.mark.parametrize("kind", ["a", "b"])
def test_records_equal_the_restatement(kind, gen_dir):
    ref = tu.reference_records(kind)
    o, d = tu.reference_rays(kind)
    s = OracleScene(gen_dir, f"gen_{kind}.cli", {})
    h = s.trace(o, d)
    hit = ref["hit"]
    assert hit.sum() > 1000 and ref["in_accel"].sum() > 300
    for f in ("hit", "prim", "top", "in_accel"):
        assert np.array_equal(h[f], ref[f]), (f, np.flatnonzero(h[f] != ref[f])[:8])
    assert np.array_equal(h["args"][hit], ref["args"][hit])
    assert not h["instance"].any() and not h["bad"].any()
    assert np.array_equal(_bits(h["t"]), _bits(ref["t"]))  # bit for bit, the +Inf of a miss included
    assert np.array_equal(_bits(h["pos"]), _bits(ref["pos"]))
    with np.errstate(all="ignore"):
        rel = np.abs(h["normal"] - ref["normal"]) / np.maximum(np.abs(h["normal"]), np.abs(ref["normal"]))
    rel = np.where(h["normal"] == ref["normal"], 0.0, rel)
    print(kind, "worst normal difference", rel.max())
    assert rel.max() <= NORMAL_TOL
    # the entry's own gap (over the candidates the reference's loops see) is above any tolerance's ceiling,
    # as the BVH-free candidate_gap of the restatement is (test_gpu_trace.py)
    assert (h["gap"][hit] > 1e-9).all()
    for j, tmax in enumerate(tu.TMAX):
        occ = s.occluded(o, d, tmax)
        assert np.array_equal(occ, ref["occ"][j]), (tmax, np.flatnonzero(occ != ref["occ"][j])[:8])


SHADE_SCENES = ["c3shinyBall.cli", "c2clear.cli", "p2_t03.cli", "p2_t05.cli"]  # mirrors, glass, keyed time, disk light


def _fov(cli):
    for line in (scenes.SCENE_DIR / cli).read_text().splitlines():
        t = line.split()
        if t and t[0] == "fov":
            return float(t[1])
    raise AssertionError(cli)


def _jd2i(x):
    x = np.where(np.isnan(x), 0.0, x)
    return np.trunc(np.clip(x, -2147483648.0, 2147483647.0)).astype(np.int64)


def _argb(c):
    """color_argb (myObjShader.java:671) of fp64 colours [n, 3]."""
    q = _jd2i(c * 255) & 0xFFFFFFFF
    v = ((255 << 24) + ((q[:, 0] << 16) & 0xFFFFFFFF) + ((q[:, 1] << 8) & 0xFFFFFFFF) + q[:, 2]) & 0xFFFFFFFF
    return v.astype(np.uint32).view(np.int32)


@pytest.mark.parametrize("cli", SHADE_SCENES)
def test_shade_reproduces_the_render(cli):
    W = H = 48
    seed = 0x5EED0001
    s = OracleScene(scenes.SCENE_DIR, cli, scenes.prepare(cli))
    rgb, argb, _ = s.render(W, H, spp=1, seed=seed)
    o, d = tu.camera_rays(W, H, _fov(cli))
    c, st = s.shade(o, d, seed=seed, first_key=0, sample=0)
    assert not st.any() and len(np.unique(argb)) > 1
    assert np.array_equal(c.astype(np.float32).view(np.uint32), rgb.reshape(-1, 3).view(np.uint32))
    assert np.array_equal(_argb(c), argb.reshape(-1))
    # the key matters where the scene draws from it
    if cli in ("p2_t03.cli", "p2_t05.cli"):
        assert not np.array_equal(s.shade(o, d, seed=seed, first_key=W * H, sample=0)[0], c)


@pytest.mark.parametrize("name", ["gen_a", "gen_b", "gen_prims"])
def test_records_do_not_depend_on_the_order(name, gen_dir):
    """Planar objects re-normalise their stored normal in place in the reference; the
    oracle hands every ray first-hit state, so a batch and its reverse agree, each ray under its own key."""
    s = OracleScene(gen_dir, f"{name}.cli", {})
    if name == "gen_prims":
        o, d = tu.shell_rays(2048)
    else:
        o, d = tu.reference_rays(name[-1])
    a = s.trace(o, d, seed=5, first_key=0, threads=1)
    n = len(o)
    rev = {f: np.empty_like(v) for f, v in a.items()}
    for i in range(n - 1, -1, -1):  # one ray per call keeps ray i's key first_key + i
        r = s.trace(o[i:i + 1], d[i:i + 1], seed=5, first_key=i, threads=1)
        for f in RECORD_FIELDS:
            rev[f][i] = r[f][0]
    assert _same(a, rev) == []
    assert _same(a, s.trace(o, d, seed=5, first_key=0, threads=4)) == []
    occ = s.occluded(o, d, 8.0, seed=5, threads=1)
    for i in range(511, -1, -1):
        assert s.occluded(o[i:i + 1], d[i:i + 1], 8.0, seed=5, first_key=i, threads=1)[0] == occ[i], i


def test_rejection_table(gen_dir):
    s = OracleScene(gen_dir, "gen_a.cli", {})
    o, d = tu.reference_rays("a")
    o, d = o[:300], d[:300]
    good = s.trace(o, d)
    good_occ = s.occluded(o, d, 8.0)
    ob, db, is_bad = tu.spoil(o, d)
    h = s.trace(ob, db)
    assert np.array_equal(h["bad"], is_bad)
    assert not h["hit"][is_bad].any() and np.isposinf(h["t"][is_bad]).all()
    assert (h["prim"][is_bad] == -1).all() and (h["top"][is_bad] == -1).all()
    assert not h["pos"][is_bad].any() and not h["normal"][is_bad].any() and not h["fp"][is_bad].any()
    for f in RECORD_FIELDS:
        assert np.array_equal(_bits(h[f][~is_bad]), _bits(good[f][~is_bad])), f
    tmax = np.full(300, 8.0)
    tmax[10] = np.nan  # a NaN tmax rejects the ray in either query mode
    is_bad[10] = True
    occ = s.occluded(ob, db, tmax)
    assert np.array_equal(occ == 2, is_bad) and np.array_equal(occ[~is_bad], good_occ[~is_bad])
    assert np.array_equal(s.trace(ob, db, tmax=tmax)["bad"], is_bad)
    c, st = s.shade(ob, db)
    is_bad[10] = False
    assert np.array_equal(st == 2, is_bad) and not c[is_bad].any() and set(np.unique(st)) == {0, 2}


def test_gen_prims_is_not_degenerate(gen_dir):
    s = OracleScene(gen_dir, "gen_prims.cli", {})
    info = s.info()
    assert info["objects"] == 12 and info["prims"] == len(tu.GEN_PRIMS_TYPES) == 14
    o, d = tu.shell_rays(2048)
    r = s.trace(o, d, seed=tu.SEED)
    ob, db, _ = tu.bounce_rays(o, d, r)
    b = s.trace(ob, db, seed=tu.SEED)
    oi, di, _ = tu.inside_rays(lambda o_, d_: s.trace(o_, d_, seed=tu.SEED), o, d, r, tu.GEN_PRIMS_CLOSED)
    i = s.trace(oi, di, seed=tu.SEED)
    assert 0.05 <= r["hit"].mean() <= 0.95 and 0.05 <= b["hit"].mean() and i["hit"].mean() >= 0.05
    occ = s.occluded(o, d, 8.0)
    assert 0.05 <= occ.mean() <= 0.95
    prim = np.concatenate([x["prim"][x["hit"]] for x in (r, b, i)])
    args = np.concatenate([x["args"][x["hit"]] for x in (r, b, i)])
    count = np.bincount(prim, minlength=14)
    print("winners per prim", count.tolist())
    assert (count >= 20).all(), count
    for p, want in tu.GEN_PRIMS_ARGS.items():
        assert set(args[prim == p].tolist()) == want, (tu.GEN_PRIMS_TYPES[p], set(args[prim == p].tolist()))
    tops = np.concatenate([x["top"][x["hit"]] for x in (r, b, i)])
    assert np.array_equal(np.concatenate([x["in_accel"][x["hit"]] for x in (r, b, i)]), tops == 9)
    assert np.array_equal(np.concatenate([x["instance"][x["hit"]] for x in (r, b, i)]), tops >= 10)
    # an instance with `shdr` reports its own material, one without the base's
    fp = np.concatenate([x["fp"][x["hit"]] for x in (r, b, i)])
    assert (fp[tops == 10][:, :3] == [.9, .9, .9]).all() and (fp[tops == 11][:, :3] == [.9, .5, .1]).all()
    assert len(np.unique(fp, axis=0)) == 12  # twelve materials, every one hit
    assert math.isinf(r["t"][~r["hit"]][0])
