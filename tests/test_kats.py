"""Reference-independent known answers (tests/golden/kats.json, derived by tests/golden/make_kats.py
in plain float64 Python from the Java formulas, without the oracle or the product): the glass
shaders (calcSimpleTransClr, calcTransClr with a real Fresnel split), the spot fall-off band and
disk-light sampling; since round 5 C3's BVH path in miniature (a translated 12-triangle myBVH: the
root's dropped element Q1, the double leaf transform Q4, a mirror ray starting inside the root box
Q2, shadow rays from the ghost point), a bilinear image texel and a k = 5 photon irradiance over
hand-placed photons; and one scene per procedural texture kind (noise, wood, wood2, marble, stone with each
distance function), six pixels each, derived from the Java's texture handlers -- at 300 x 300, 1 spp. The oracle (CPU) and the HIP path (-m gpu) must reproduce
each pixel: float32 RGB within 2e-6 of the derived double colour for the first five (host libm vs
fdlibm trig: an ulp), 1e-6 for the round-5 ones, and the ARGB int exactly (the script keeps every
channel 1e-9 away from a truncation step)."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

from distraytracer_old_amd import scenes

GOLDEN = Path(__file__).resolve().parent / "golden"
KATS = json.loads((GOLDEN / "kats.json").read_text())
TOL = 2e-6
TOL_R5 = 1e-6  # the round-5 KATs (BVH, texel, photon irradiance)
R5 = {"bvh_q1_q2_q4_tile", "bvh_q4_ghost_blocked", "earth_bilinear_texel", "photon_irradiance_k5"}
# the procedural-texture KATs with no libm call on their path beyond sqrt (float noise; the Euclidean altLinROI
# stone) go with them; wood, wood2, marble (sin) and the Manhattan stone (log) keep TOL
R5 |= {"%s_%d" % (k, i) for k in ("noise", "stone_euclid") for i in range(6)}


def _make_kats():
    spec = importlib.util.spec_from_file_location("make_kats", GOLDEN / "make_kats.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _scene(kat, tmp_path):
    """(scene_dir, cli, textures) of a KAT's scene; trTrans_plain.cli is written to tmp_path, the
    KAT-only scenes live in tests/golden/kat_scenes."""
    if kat["cli"] == "trTrans_plain.cli":
        (tmp_path / kat["cli"]).write_text(_make_kats().scene_text(kat["cli"]))
        return tmp_path, kat["cli"], {}
    if (GOLDEN / "kat_scenes" / kat["cli"]).exists():
        return GOLDEN / "kat_scenes", kat["cli"], {}
    return scenes.SCENE_DIR, kat["cli"], scenes.prepare(kat["cli"])


def _photons(kat):
    return np.asarray(kat["photons"]["pos"], dtype=np.float64), np.asarray(kat["photons"]["pwr"], dtype=np.float64)


def _check(kat, rgb, argb):
    got = rgb[0, kat["col"]].astype(np.float64)
    tol = TOL_R5 if kat["name"] in R5 else TOL
    assert np.abs(got - np.asarray(kat["rgb"])).max() <= tol, (kat["name"], got, kat["rgb"])
    assert int(argb[0, kat["col"]]) == kat["argb"], (kat["name"], hex(int(argb[0, kat["col"]]) & 0xFFFFFFFF))


def test_kat_fixture_is_the_derivation():
    """kats.json is what make_kats.py derives (the script is the fixture's source of truth)."""
    m = _make_kats()
    assert R5 <= {k["name"] for k in KATS["kats"]}
    for kat in KATS["kats"]:
        sc = m.kat_scene(kat, KATS["W"], KATS["H"])
        assert sc.pixel(kat["row"], kat["col"], KATS["seed"]) == kat["rgb"], kat["name"]


@pytest.mark.parametrize("kat", KATS["kats"], ids=[k["name"] for k in KATS["kats"]])
def test_oracle_reproduces_kat(kat, tmp_path):
    from oracle.oracle import OracleScene

    d, cli, tex = _scene(kat, tmp_path)
    o = OracleScene(d, cli, tex)
    if "photons" in kat:
        o.set_photons(*_photons(kat))
    rgb, argb, _ = o.render(KATS["W"], KATS["H"], spp=1, seed=KATS["seed"], rows=(kat["row"], kat["row"] + 1))
    _check(kat, rgb, argb)


@pytest.mark.gpu
@pytest.mark.parametrize("kat", KATS["kats"], ids=[k["name"] for k in KATS["kats"]])
def test_gpu_reproduces_kat(kat, tmp_path):
    from distraytracer_old_amd import rt

    d, cli, tex = _scene(kat, tmp_path)
    with rt.Scene.load_cli(cli, scene_dir=d, textures=tex) as g:
        if "photons" in kat:
            g.set_photons(*_photons(kat))
        rgb, argb = g.render(KATS["W"], KATS["H"], spp=1, seed=KATS["seed"], rows=(kat["row"], kat["row"] + 1))
    _check(kat, rgb, argb)
