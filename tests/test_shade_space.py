"""The shading space, CPU side (tests/shade_util.py has the fixtures and what each is named for): the proof
that the fixtures of test_gpu_shade_space.py are worth comparing on, on any machine.

1. Restatement == oracle. On every fixture's check rays (all 4096 of them, every family; a stride of 1024
   for glass_full, whose trees are full), both samples, the plain-Python restatement's colour equals
   OracleScene.shade within 1e-12 absolute, NaN equal to NaN. Expected: bit-equal, or a last ulp of host
   libm against fdlibm trig (measured here: 0 to 2.4e-15, the largest on glass_below_one).
2. Reach floors. From the restatement's events on those rays every branch a fixture is named for is taken by
   at least 32 rays (8 for the depth gate and for the deepest two-child level): a condition on the fixture,
   so that one which stops reaching its branch fails here instead of quietly testing less on the GPU.
3. Term floors. Per branch a sibling scene with that one thing changed (specular colour 0, the spot made a
   point light, krefl 0, the index changed, the inner sphere's medium removed): on the rays that reach the
   branch, the oracle's colour differs between the two scenes by more than 1e-6 on at least 32 rays. This is
   what lets the tight GPU tolerance mean something: a kernel that dropped the term would move those rays
   by more than any bound the GPU test asserts."""
import numpy as np
import pytest

from tests import shade_util as su

TOL = 1e-12
MOVED = 1e-6


@pytest.fixture(scope="module")
def oracle_of(tmp_path_factory):
    from oracle.oracle import OracleScene

    d = tmp_path_factory.mktemp("shade_space")
    su.write_all(d)
    cache = {}

    def colours(name, text=None, sample=0):
        """The oracle's colours of fixture `name`'s rays in its own scene, or in the sibling `text`."""
        key = (name, text, sample)
        if key not in cache:
            cli = name + ".cli"
            if text is not None:
                cli = "sibling_%d.cli" % len(cache)
                (d / cli).write_text(text)
            fx = su.fixture(name)
            o = OracleScene(d, cli, {})
            cache[key] = o.shade(fx.o, fx.d, seed=su.SEED, first_key=su.FIRST_KEY, sample=sample)
            o.close()
        return cache[key]
    return colours


def test_fixtures_stay_inside_their_limits():
    assert len(su.NAMES) == 11
    for n in su.NAMES:
        fx = su.fixture(n)
        assert 512 <= len(fx.check) <= len(fx.o) <= 4096
        assert np.isfinite(fx.o).all() and np.isfinite(fx.d).all() and fx.d.any(1).all()
        assert set(fx.family) == ({"R"} if not fx.spheres else {"R", "I", "N"})
    lights = [line.split()[0] for line in su.fixture("light_mix").text.splitlines() if "light" in line.split()[0]]
    assert len(lights) >= 7 and {"point_light", "spotlight", "disk_light"} == set(lights)
    assert "light" not in su.fixture("no_lights").text


@pytest.mark.parametrize("name", su.NAMES)
def test_restatement_equals_the_oracle(name, oracle_of):
    fx = su.fixture(name)
    for sample in su.SAMPLES:
        want, st = oracle_of(name, sample=sample)
        assert not st.any()
        got, _ = su.restated(name, sample)
        dev = su.deviation(got, want[fx.check])
        print(f"{name} sample {sample}: {len(fx.check)} rays, worst |restatement - oracle| {dev.max():.3g}, "
              f"NaN colours {int(np.isnan(want).any(1).sum())}")
        assert dev.max() <= TOL, (name, sample, np.argwhere(dev > TOL)[:4].tolist())
    if name == "light_mix":  # two samples so that the disk lights' points differ
        assert (np.abs(oracle_of(name, sample=0)[0] - oracle_of(name, sample=3)[0]).max(1) > MOVED).sum() >= 32


@pytest.mark.parametrize("name,branch", [(n, b) for n in su.NAMES for b in su.fixture(n).reach])
def test_reach_floor(name, branch):
    floor = su.fixture(name).reach[branch][1]
    count = int(su.reached(name, branch).sum())
    print(f"{name}: {branch}: {count} rays (floor {floor})")
    assert count >= floor


@pytest.mark.parametrize("name,k", [(n, k) for n in su.NAMES for k in range(len(su.fixture(n).siblings))])
def test_term_floor(name, k, oracle_of):
    fx = su.fixture(name)
    what, text, branch = fx.siblings[k]
    assert text != fx.text
    a, _ = oracle_of(name)
    b, _ = oracle_of(name, text=text)
    moved = (su.deviation(a, b).max(1) > MOVED)[fx.check] & su.reached(name, branch)
    print(f"{name}: {what}: moves {int(moved.sum())} of the {int(su.reached(name, branch).sum())} rays on [{branch}]")
    assert moved.sum() >= 32


def test_every_fixture_has_a_term_floor_and_every_listed_change_is_used():
    changes = " ".join(s[0] for n in su.NAMES for s in su.fixture(n).siblings)
    for word in ("specular colour 0", "point light", "krefl 0", "index", "medium removed"):
        assert word in changes, word
    assert all(su.fixture(n).siblings for n in su.NAMES)
