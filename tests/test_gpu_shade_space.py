"""Lights, the specular term, the Fresnel split and the shading tree over their branch space, on the GPU, against
the oracle. The fixtures are tests/shade_util.py's; tests/test_shade_space.py proves on the CPU that each reaches
the branches it is named for, that each branch moves the colour by more than 1e-6 on at least 32 rays, and that
the oracle's colours on them are the plain-Python restatement's to 1e-12.

A. Caller rays. Scene.shade on every fixture's 4096 rays (families R, I, N), samples 0 and 3, flags 0,
   TRACE_GENERIC, TRACE_NOCULL, TRACE_SORT, against OracleScene.shade: equal status bytes, no ray left out, and the
   modes equal to each other bit for bit.
   - No specular term on any path (spot_bands, light_mix, no_lights, the five glass fixtures, and in phong_row
     every ray whose hit is the floor, the exponent-0 sphere or nothing): the same fp64 operations in the same
     order with shared trig. Bit equality, NaN equal to NaN.
   - Specular term present: the deviation is the phong shortcut (H normalised with one reciprocal, integer
     exponents 0..1024 by squaring) and ocml's pow on the pow_call path. Asserted: MARGIN = 8 x the worst
     absolute deviation measured on one MI355X, per exponent of phong_row and per remaining fixture (the factor
     is the project's margin for a last-ulp effect seen on one GPU and one ocml version, as TOL["normal"] of
     test_gpu_trace.py); no bound may exceed 1e-9.
B. Frames. Every fixture at 37 x 23 and 23 x 37 (no other oracle comparison of the suite has H > W), spp 1 and 5,
   render flags 0, GENERIC, SHCOMPACT, NOWAVECULL, WAVEFRONT and PIXEL_WAVES (spp 5 only), each against
   OracleScene.render by parity.assert_exact_decisions and equal to flags 0 bit for bit in rgb and ARGB.
C. Counters. render_count(RENDER_NOCULL) at 37 x 23, spp 2: camera, shadow, refl, refr and light equal the
   oracle's on every fixture; light - shadow > 0 on spot_bands is the skipped light seen from the kernel's side.
D. Cameras. `mirrors` under `ortho 6 4`, `fisheye 120` and `lens 0.1 6` at both sizes, spp 1 and 4, against the
   oracle by the same rule: the reference scenes' ortho parameters are square and their ortho and lens frames
   are only rendered square, so swapped per-row / per-column steps would pass everything else.

Measured (one MI355X; worst |GPU - oracle| of a colour channel over both samples, the same in all four modes,
rounded up in the third digit; the bound asserted is 8 x this, the largest 3.4e-12):
   phong_row, rays on the sphere of exponent
       1     square    2.23e-16        33    square    5.33e-15      1025  pow_call  2.12e-13
       2     square    3.34e-16        160   square    2.71e-14      2000  pow_call  4.23e-13
       3     square    5.56e-16        1023  square    1.98e-13      -2    pow_call  0 (mostly clamped to 1)
       7.25  pow_call  1.56e-15        1024  square    1.99e-13
       0.5   pow_call  2.23e-16
   mirrors   (exponent 40, square, under up to six mirror levels)    4.56e-15
   tri_only  (exponent 12.5, pow_call)                                1.56e-15
   every ray without a specular term on its path: 0 (bit-equal), NaN colours: none arise (a NaN refraction
   ray misses everything and a NaN tr spawns no child, so the NaN never reaches a colour)
For orientation: squaring an exponent e stays near 9 e 2^-53 relative to the term (1e-12 at 1024)."""
import numpy as np
import pytest

from distraytracer_old_amd import rt
from tests import parity
from tests import shade_util as su

pytestmark = pytest.mark.gpu

MODES = {"packet": 0, "generic": rt.TRACE_GENERIC, "nocull": rt.TRACE_NOCULL, "sort": rt.TRACE_SORT}
MARGIN = 8
CEILING = 1e-9
# worst absolute deviation of a colour channel from the oracle's, per phong exponent (phong_row: rays whose hit is
# that exponent's sphere) and per remaining fixture with a specular term; the pow_shade path in the comment
MEASURED_PHONG = {
    1: 2.23e-16,     # square
    2: 3.34e-16,     # square
    3: 5.56e-16,     # square
    7.25: 1.56e-15,  # pow_call
    0.5: 2.23e-16,   # pow_call
    33: 5.33e-15,    # square
    160: 2.71e-14,   # square
    1023: 1.98e-13,  # square
    1024: 1.99e-13,  # square
    1025: 2.12e-13,  # pow_call
    2000: 4.23e-13,  # pow_call
    -2: 0.0,         # pow_call: bit-equal on all 469 rays ((hdp^2)^-2 >= 1: most lit channels are clamped to exactly 1)
}
MEASURED = {
    "mirrors": 4.56e-15,   # exponent 40: square, seen through up to six mirror levels
    "tri_only": 1.56e-15,  # exponent 12.5: pow_call
}

SIZES = ((37, 23), (23, 37))
RENDER_FLAGS = {"generic": rt.RENDER_GENERIC, "shcompact": rt.RENDER_SHCOMPACT, "nowavecull": rt.RENDER_NOWAVECULL,
                "wavefront": rt.RENDER_WAVEFRONT, "pixel_waves": rt.RENDER_PIXEL_WAVES}
CAMERAS = {"ortho": "ortho 6 4", "fisheye": "fisheye 120", "lens": "fov 60\nlens 0.1 6"}


class Case:
    """One fixture on both sides, with the oracle's colours of its rays for both samples (computed once)."""

    def __init__(self, d, name, cli=None):
        from oracle.oracle import OracleScene

        self.fx = su.fixture(name)
        cli = cli or name + ".cli"
        self.o = OracleScene(d, cli, {})
        self.g = rt.Scene.load_cli(cli, scene_dir=d, textures={})
        self._want = {}

    def want(self, sample):
        if sample not in self._want:
            rgb, st = self.o.shade(self.fx.o, self.fx.d, seed=su.SEED, first_key=su.FIRST_KEY, sample=sample)
            rgb.setflags(write=False)
            self._want[sample] = (rgb, st)
        return self._want[sample]

    def close(self):
        self.g.close()
        self.o.close()


@pytest.fixture(scope="module")
def case_of(tmp_path_factory):
    d = tmp_path_factory.mktemp("shade_space_gpu")
    su.write_all(d)
    for cam, line in CAMERAS.items():
        text = su.fixture("mirrors").text
        assert text.startswith("fov 60\n")
        (d / ("mirrors_%s.cli" % cam)).write_text(text.replace("fov 60", line, 1))
    cache = {}

    def get(name, cam=None):
        if (name, cam) not in cache:
            cache[name, cam] = Case(d, name, "%s_%s.cli" % (name, cam) if cam else None)
        return cache[name, cam]

    yield get
    for c in cache.values():
        c.close()


# ---- A. caller rays ------------------------------------------------------------------------------------------
def _groups(c):
    """[(label, ray mask, measured worst or None for bit equality)] of a fixture's rays."""
    fx = c.fx
    every = np.ones(len(fx.o), dtype=bool)
    if not fx.specular:
        return [("all", every, None)]
    if fx.name != "phong_row":
        return [("all", every, MEASURED[fx.name])]
    prim = c.o.trace(fx.o, fx.d, seed=su.SEED, first_key=su.FIRST_KEY)["prim"]  # krefl 0: the first hit is the only one
    out = [("floor, exponent 0 or a miss", ~np.isin(prim, [k for k, e in fx.prims.items() if e != 0]), None)]
    for k, e in fx.prims.items():
        if e != 0:
            out.append(("exponent %r (%s)" % (e, su.pow_path(e)), prim == k, MEASURED_PHONG[e]))
    assert np.sum([m for _, m, _ in out], axis=0).tolist() == [1] * len(fx.o)
    return out


@pytest.mark.parametrize("name", su.NAMES)
def test_caller_rays_match_the_oracle(name, case_of):
    c = case_of(name)
    fx = c.fx
    groups = _groups(c)
    failures = []
    for sample in su.SAMPLES:
        want, wst = c.want(sample)
        assert not wst.any() and len(np.unique(want[~np.isnan(want).any(1)], axis=0)) > 16
        first = None
        for mode, fl in MODES.items():
            got, gst = c.g.shade(fx.o, fx.d, seed=su.SEED, first_key=su.FIRST_KEY, sample=sample, flags=fl)
            assert got.shape == want.shape and np.array_equal(gst, wst), (name, sample, mode)
            if first is None:
                first = got
            elif got.tobytes() != first.tobytes():
                failures.append((sample, mode, "differs from packet mode on rays", np.flatnonzero((got != first).any(1))[:8].tolist()))
        dev = su.deviation(first, want).max(1)
        for label, mask, measured in groups:
            assert mask.sum() >= 32, (name, label)
            worst = float(dev[mask].max())
            print(f"{name} sample {sample} [{label}]: {int(mask.sum())} rays, worst |GPU - oracle| {worst:.3g}, "
                  f"differing rays {int((dev[mask] > 0).sum())}, NaN colours {int(np.isnan(want[mask]).any(1).sum())}")
            if measured is None:
                if not su.same_or_nan(first[mask], want[mask]).all():
                    failures.append((sample, label, "not bit-equal", worst, np.flatnonzero(mask & (dev > 0))[:8].tolist()))
            else:
                assert MARGIN * measured <= CEILING, (label, measured)
                if not worst <= MARGIN * measured:
                    failures.append((sample, label, "beyond 8 x measured", worst, measured))
    assert not failures, failures


# ---- B. frames -----------------------------------------------------------------------------------------------
def _frames_against_the_oracle(c, what, spps, flags):
    failures = []
    for W, H in SIZES:
        for spp in spps:
            ro, ao, _ = c.o.render(W, H, spp=spp)
            assert ro.shape == (H, W, 3) and len(np.unique(ao)) > 8, (what, W, H)
            base = None
            for mode, fl in [("default", 0)] + list(flags.items()):
                if mode == "pixel_waves" and spp < 2:
                    continue
                rg, ag = c.g.render(W, H, spp=spp, flags=fl)
                cmp = parity.compare(rg, ag, ro, ao)
                print(what, f"{W}x{H} spp {spp} {mode}: max |d| {cmp['max_abs']:.3g}, mismatches {cmp['mismatch']}, "
                      f"ARGB mismatches {cmp['argb_mismatch_on_good']}")
                if cmp["mismatch"] or cmp["argb_mismatch_on_good"]:
                    failures.append((W, H, spp, mode, cmp))
                if base is None:
                    base = (rg, ag)
                elif not (np.array_equal(rg.view(np.uint32), base[0].view(np.uint32)) and np.array_equal(ag, base[1])):
                    failures.append((W, H, spp, mode, "differs from the default flags"))
    return failures


@pytest.mark.parametrize("name", su.NAMES)
def test_frames_match_the_oracle(name, case_of):
    c = case_of(name)
    timed, counted = c.g.variant()
    print(name, "variant masks (timed, counted)", timed, counted)
    if name == "tri_only":
        assert timed == 0  # triangles, point lights, mirrors: the benchmark's kernel (FrameR)
    failures = _frames_against_the_oracle(c, name, (1, 5), RENDER_FLAGS)
    assert not failures, failures


# ---- C. counters ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", su.NAMES)
def test_counters_equal_the_oracles(name, case_of):
    c = case_of(name)
    W, H = SIZES[0]
    _, _, sg = c.g.render_count(W, H, spp=2, flags=rt.RENDER_NOCULL)
    _, _, so = c.o.render(W, H, spp=2)
    keys = ("camera", "shadow", "refl", "refr", "light")
    print(name, {k: (sg[k], so[k]) for k in keys})
    assert {k: sg[k] for k in keys} == {k: so[k] for k in keys}
    assert sg["camera"] == 2 * W * H
    if name == "spot_bands":
        assert sg["light"] - sg["shadow"] > 0  # lights skipped before their shadow ray
    if name == "no_lights":
        assert sg["light"] == sg["shadow"] == 0 and sg["refl"] > 0


# ---- D. cameras ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", list(CAMERAS))
def test_cameras_on_frames_that_are_not_square(cam, case_of):
    c = case_of("mirrors", cam)
    failures = _frames_against_the_oracle(c, "mirrors under " + CAMERAS[cam].replace("\n", " / "), (1, 4), {"generic": rt.RENDER_GENERIC})
    assert not failures, failures
