"""The procedural and image textures over their parameter space, HIP against the oracle.

Scenes (tests/tex_util.py): gen_tex_perlin (noise, marble, wood, wood2: argument forms, octaves, period and pi
multipliers, turbMult 0, useFwdTrans on identity / translated / rotated and scaled spheres, custom colour
lists), gen_tex_stone (distance function x ROI function 0..9 x numPtsDist 1, 2, 3, 8, and densities, mortar
thresholds, colour lists, the `pdf edge` tile) and gen_tex_image (generated textures of 1 x 1 to 64 x 64 on
every primitive kind that can carry one, planar (u, v) outside [0, 1], poles and seam). One primitive per
material, RAYS rays per tile, about 10 k rays a scene, one load each.

What is asserted, per scene, for rt_shade_rays under flags 0, TRACE_SORT and TRACE_GENERIC and samples 0 and 3,
with the oracle's colours under equal keys as the reference, on every ray (NaN channels -- the reference's
0 / 0 texture coordinates on a 1-texel-high image, a parallelogram quad and the plane -- compare as -1):
 1. the project's rule per tile: parity.compare, then assert_exact_decisions (a failure names the material);
 2. |d| <= 1e-9 per channel on the float64 colours. 1e-9 is the ceiling this suite puts on any tolerance
    (tests/test_gpu_prims.py); a texture is a few dozen fp64 roundings and libm ulps (pow, log in the ROI
    functions, fdlibm sin on both sides) on float noise that is bit-equal or wholly different, so agreement is
    expected near 1e-14 and the smallest term a wrong texture drops (the last of 16 octaves) is 1e-4. The
    worst |d| per kind is printed; DESIGN.md records the measured figures;
 3. the render kernel's own variants: each scene at 32 x 32, 2 spp, default and RENDER_GENERIC, against the
    oracle's frame by the same rule, the variant mask holding FT_TEX (and FT_CELL for the stone scene).
The conditions that keep this from passing on nothing are asserted on the oracle's output by
tests/test_textures.py::test_conditions_hold_on_the_oracle (no GPU needed); the cheap ones are repeated here."""
import numpy as np
import pytest

from distraytracer_old_amd import rt
from tests import parity
from tests import tex_util as tx
from tests.test_gpu_shade import _pack

pytestmark = pytest.mark.gpu

FT_TEX, FT_CELL = 2, 512  # csrc/trace_kernels.h
TIGHT = 1e-9
MODES = {"packet": 0, "sort": rt.TRACE_SORT, "generic": rt.TRACE_GENERIC}


@pytest.fixture(scope="module")
def case_of(tmp_path_factory):
    d = tmp_path_factory.mktemp("tex_scenes")
    cache = {}

    def get(name):
        if name not in cache:
            c = tx.OracleCase(tx.GENERATORS[name], d)
            c.g = rt.Scene.load_cli(c.cli, scene_dir=d, textures=c.sc.textures)
            cache[name] = c
        return cache[name]

    yield get
    for c in cache.values():
        c.g.close()
        c.close()


@pytest.mark.parametrize("name", list(tx.GENERATORS))
def test_radiance_matches_the_oracle(name, case_of):
    c = case_of(name)
    o, d = c.origin, c.dir_
    own = c.on == c.tile
    failures, worst = [], {}
    for t in c.sc.tiles:  # cheap repeats of the conditions (the full set: tests/test_textures.py)
        m = (c.tile == t.index) & (c.family == "tile")
        assert (own & m).sum() >= 48, t.name
        if t.kind != "plain" and not t.facts.get("nan"):
            assert len(np.unique(c.want[0][0][own & m], axis=0)) >= 20, t.name
    compared = 0
    for sample in (0, 3):
        want, wst = c.want[sample]
        assert (wst == 0).all()
        for mode, fl in MODES.items():
            got, gst = c.g.shade(o, d, seed=tx.SEED, first_key=tx.FIRST_KEY, sample=sample, flags=fl)
            assert np.array_equal(gst, wst), (name, mode)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (name, mode, "NaN channels differ")
            a, b = tx.clean(got), tx.clean(want)
            diff = np.abs(a - b).max(1)
            for t in c.sc.tiles:
                m = c.tile == t.index
                cmp = parity.compare(a[m][:, None, :], _pack(a[m])[:, None], b[m][:, None, :], _pack(b[m])[:, None])
                try:
                    parity.assert_exact_decisions(cmp)
                except AssertionError:
                    failures.append((t.name, "sample", sample, mode, "parity rule", cmp["max_abs"], cmp["mismatch"],
                                     cmp["argb_mismatch_on_good"]))
                w = float(diff[m].max())
                worst[t.kind] = max(worst.get(t.kind, 0.0), w)
                if not w <= TIGHT:
                    k = np.flatnonzero(m)[np.argmax(diff[m])]
                    failures.append((t.name, "sample", sample, mode, "|d|", w, "ray", int(k), got[k].tolist(), want[k].tolist()))
                compared += int(m.sum())
    print(name, "worst |d| per kind", worst)
    assert compared == len(o) * 2 * len(MODES)  # no ray is left out
    assert not failures, failures[:12]


@pytest.mark.parametrize("name", list(tx.GENERATORS))
def test_render_variants_match_the_oracle(name, case_of):
    c = case_of(name)
    W, spp = 32, 2
    ro, ao, _ = c.o.render(W, W, spp=spp, seed=tx.SEED)
    assert len(np.unique(ao)) > 100  # the frame shows the tiles
    for what, fl in (("specialised", 0), ("generic", rt.RENDER_GENERIC)):
        timed, counted = c.g.variant(fl)
        need = FT_TEX | (FT_CELL if name == "gen_tex_stone" else 0)
        assert timed & need == need and counted & need == need, (name, what, timed, counted)
        rg, ag = c.g.render(W, W, spp=spp, seed=tx.SEED, flags=fl)
        assert np.array_equal(np.isnan(rg), np.isnan(ro)), (name, what)
        cmp = parity.compare(tx.clean(rg), ag, tx.clean(ro), ao)
        print(name, what, cmp)
        parity.assert_exact_decisions(cmp)


def test_nine_roi_points_are_refused(tmp_path):
    """The sorted register list holds 8 distances: numPtsDist = 9 is refused at load, by name."""
    text = tx.gen_tex_stone().text.replace("stone 6.0 1 1 2 ", "stone 6.0 1 1 9 ", 1)
    assert " 1 1 9 " in text
    (tmp_path / "nine.cli").write_text(text)
    for load in (lambda: rt.Scene.load_cli("nine.cli", scene_dir=tmp_path, textures={}),
                 lambda: rt.inspect_cli("nine.cli", scene_dir=tmp_path, textures={})):
        with pytest.raises(rt.RTError, match="stone: more than 8 ROI points unsupported"):
            load()
    (tmp_path / "eight.cli").write_text(text.replace(" 1 1 9 ", " 1 1 8 ", 1))
    assert rt.inspect_cli("eight.cli", scene_dir=tmp_path, textures={})["objects"] > 0
