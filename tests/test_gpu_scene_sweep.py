"""Every reference scene renders as the oracle does: one 64 x 64 frame per scenes/*.cli file that no other
GPU test compares with the oracle, by the rule of tests/parity.py (per-channel TOL, then exact decisions).

The directory is partitioned into three explicit parts, and a CPU test asserts the partition:
COVERED  -- already rendered against the oracle elsewhere (tests/test_gpu_parity.py);
EXCLUDED -- not scenes: files that other scenes `read` or that draw nothing on their own (a CPU test asserts
            that the oracle's frame of each has exactly one colour), one scene whose texture does not exist,
            and the generated bun69k.cli;
the rest -- SWEEP, built from the directory listing, so a new scene file is picked up by itself."""
import re
import shutil

import numpy as np
import pytest

from distraytracer_old_amd import rt, scenes
from tests.parity import assert_exact_decisions, compare

SEED = 0x5EED0001
W = H = 64
PHOTONS = 20000  # the *_photons count of the temporary copy (t08 says 80 000 000: never run as written)

# rendered against the oracle by tests/test_gpu_parity.py
COVERED = {
    "t01.cli", "c3shinyBall.cli", "c3_bun69k.cli", "plnts3ColsBunnies.cli",                  # C1 .. C4
    "old_t07.cli", "old_t10.cli", "planets3Ortho.cli",                                       # test_camera_scenes_parity
    "p2_t05.cli", "p2_t07.cli", "c2clear.cli", "p2_t03.cli", "p3_t09.cli", "p4_t05.cli", "p4_t06_2.cli",  # test_feature_scenes_parity
    *(f"p4_st0{i}.cli" for i in range(1, 10)),                                               # test_stone_parity
    "p3_t01.cli", "p3_t02.cli", "p3_t03.cli", "p4_t02.cli", "p4_t05Alt.cli", "p3_t10.cli", "p3_t11.cli",
    "p3_t02_sierp.cli", "p3_t11_sierp.cli",                                                  # test_instance_parity
    "t11.cli",                                                                               # test_photon_map_parity, C5
    "c2torus.cli", "old_t07a.cli", "rect_test.cli", "p4_t06Alt.cli", "c4InSphere.cli",       # test_ignored_command_scenes_parity
}
# includes and files that draw nothing: test_excluded_files_draw_nothing holds each to a one-colour frame
INCLUDES = {"box.cli", "bun500.cli", "cube.cli", "old_box.cli", "sm2TriFloor.cli", "worleyClrs.cli"}
EXCLUDED = INCLUDES | {
    "planets3backup.cli",  # its texture file does not exist (in the reference's data either)
    "bun69k.cli",          # generated input of c3_bun69k.cli, not a scene
}
ONE_COLOUR = INCLUDES | {"c2torus.cli", "rect_test.cli"}  # the last two: test_ignored_command_scenes_parity renders them

ALL = sorted(p.name for p in scenes.SCENE_DIR.glob("*.cli"))
SWEEP = [c for c in ALL if c not in COVERED and c not in EXCLUDED]


def _text(cli, scene_dir=scenes.SCENE_DIR):
    """The file's text with the files it reads (one level is all the scenes use)."""
    t = (scene_dir / cli).read_text()
    return t + "".join("\n" + (scene_dir / r).read_text() for r in scenes._reads(t) if (scene_dir / r).exists())


def _commands(text):
    return [line.split() for line in text.splitlines() if line.split() and not line.lstrip().startswith("#")]


def _spp(cli):
    """2 where the frame draws random numbers per sample (lens, disk light, moving sphere) or the file asks
    for more than one ray per pixel, else 1."""
    cmds = _commands(_text(cli))
    if any(c[0] in ("lens", "disk_light", "moving_sphere") for c in cmds):
        return 2
    return 2 if any(c[0] == "rays_per_pixel" and int(c[1]) > 1 for c in cmds) else 1


PHOTON_RE = re.compile(r"^(\s*(?:diffuse|caustic)_photons\s+)(\d+)", re.M)


def test_the_lists_partition_the_directory():
    assert len(ALL) > 100 and len(set(ALL)) == len(ALL)
    assert COVERED <= set(ALL) and EXCLUDED - {"bun69k.cli"} <= set(ALL)  # bun69k.cli is generated on demand
    assert not COVERED & EXCLUDED
    assert sorted(set(SWEEP) | COVERED | (EXCLUDED & set(ALL))) == ALL
    assert len(SWEEP) + len(COVERED) + len(EXCLUDED & set(ALL)) == len(ALL)
    # what the sweep is for: the primitive types and caustic scenes no other GPU test renders
    for cli in ("p3_t04.cli", "old_t08.cli", "t06.cli", "t07.cli", "t08.cli", "old_t04a.cli", "old_t05a.cli", "cylinder1.cli",
                "t03.cli", "t04.cli", "t05.cli", "t10.cli"):
        assert cli in SWEEP, cli
    assert _spp("p2_t06.cli") == 2 and _spp("p3_t04.cli") == 1
    assert PHOTON_RE.search((scenes.SCENE_DIR / "t08.cli").read_text()).group(2) == "80000000"


@pytest.mark.parametrize("cli", sorted(ONE_COLOUR))
def test_excluded_files_draw_nothing(cli):
    """"Include" is not a claim: the oracle's frame of every file excluded as one has exactly one colour."""
    from oracle.oracle import OracleScene

    _, argb, _ = OracleScene(scenes.SCENE_DIR, cli, scenes.prepare(cli)).render(W, H, spp=1, seed=SEED)
    assert len(np.unique(argb)) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("cli", SWEEP)
def test_scene_renders_as_the_oracle_does(cli, tmp_path):
    from oracle.oracle import OracleScene

    scene_dir, tex = scenes.SCENE_DIR, scenes.prepare(cli)
    src = (scene_dir / cli).read_text()
    photon = PHOTON_RE.search(src) is not None
    if photon:  # a temporary copy with a small photon count; k and the radius stay
        for r in scenes._reads(src):
            shutil.copy(scene_dir / r, tmp_path / r)
        (tmp_path / cli).write_text(PHOTON_RE.sub(lambda m: m.group(1) + str(PHOTONS), src))
        scene_dir = tmp_path
        assert str(PHOTONS) in (tmp_path / cli).read_text() and "80000000" not in (tmp_path / cli).read_text()
    spp = _spp(cli)
    with rt.Scene.load_cli(cli, scene_dir=scene_dir, textures=tex) as g:
        o = OracleScene(scene_dir, cli, tex)
        if photon:
            g.build_photons(SEED)
            assert g.info()["photons"] == o.build_photons(SEED)
            (gp, gw), (op, ow) = g.photons(), o.photons()
            assert np.array_equal(gp.view(np.uint64), op.view(np.uint64))
            assert np.array_equal(gw.view(np.uint64), ow.view(np.uint64))
        rg, ag = g.render(W, H, spp=spp, seed=SEED)
        ro, ao, _ = o.render(W, H, spp=spp, seed=SEED)
        c = compare(rg, ag, ro, ao)
        if c["mismatch"] or c["argb_mismatch_on_good"]:
            bad = np.argwhere(np.abs(rg.astype(np.float64) - ro).max(-1) > 1e-4)[:8]
            print(cli, spp, c, "first differing pixels (row, col)", bad.tolist())
        assert_exact_decisions(c)
        assert len(np.unique(ao)) > 1, "the frame shows nothing"
