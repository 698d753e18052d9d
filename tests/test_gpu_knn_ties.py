"""Exact distance ties at the k-th photon on the GPU (VERDICT r03 Missing #3): the device gather
must keep the photons the reference keeps. myKD_Tree.find_near (myLight.java:389-445) decides ties
by its kd-tree visit order and java.util.PriorityQueue's JDK 8 sifts; the device's counting selection
detects a lane whose k-th distance is shared across the boundary and replays find_near over the
reference's kd-tree for it (trace_kernels.h knn_java). The oracle's JavaMaxPQ is pinned against an
independent Python restatement by tests/test_knn_ties.py, on the same lattice fixture used here.

Tolerance: irradiance within 1e-12 relative everywhere (lanes without a tie across the k-th position
sum in scan order, the reference in poll order: last-ulp differences), and bit-equal where the tie
straddles the boundary (the replay sums in poll order, as the oracle)."""
import numpy as np
import pytest

from distraytracer_old_amd import rt
from oracle.oracle import OracleScene
from tests.parity import assert_exact_decisions, compare
from tests.test_knn_ties import _lattice

pytestmark = pytest.mark.gpu

PI_F = 3.1415927410125732  # (double)PConstants.PI


def _oracle_irradiance(o, pos, pwr, q, k):
    """(irradiance, straddle): straddle when photons at the neighbourhood's largest distance are
    both in and out of it -- the case only the reference's kd-tree order and heap decide."""
    idx, d2 = o.knn(q)
    if len(idx) == 0:
        return np.zeros(3), False
    s = np.zeros(3)
    for i in idx:  # poll order, farthest first (getIrradianceFromPhtnTree)
        s = s + pwr[i]
    dx, dy, dz = q[0] - pos[:, 0], q[1] - pos[:, 1], q[2] - pos[:, 2]
    all_d2 = dx * dx + dy * dy + dz * dz  # find_near's len2, same operations
    straddle = len(idx) == k and int((all_d2 == d2[0]).sum()) > int((d2 == d2[0]).sum())
    return s / (PI_F * d2[0]), straddle


@pytest.mark.parametrize("build", ["gpu", "host"])
@pytest.mark.parametrize("k", [5, 6, 13, 30])
@pytest.mark.parametrize("seed", [1, 2])
def test_gather_ties_follow_java_priority_queue(tmp_path, monkeypatch, k, seed, build):
    cli = tmp_path / "knn.cli"
    cli.write_text(f"fov 60\nbackground 0 0 0\npoint_light 0 5 0 1 1 1\ndiffuse_photons 100 {k} 10\n"
                   "diffuse .5 .5 .5 0 0 0\nsphere 1 0 0 -5\n")
    pos, pwr = _lattice(seed)
    if build == "host":
        monkeypatch.setenv("DISTRAYTRACER_PHOTON_BUILD", "host")
    g = rt.Scene.load_cli("knn.cli", scene_dir=tmp_path, textures={})
    g.set_photons(pos, pwr)
    o = OracleScene(tmp_path, "knn.cli")
    o.set_photons(pos, pwr)
    rng = np.random.default_rng(seed + 10 * k)
    lattice_q = [(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.5, 0.5, 0.0), (1.0, -1.0, 0.5), (-2.0, 1.0, 0.0)]
    qs = np.concatenate([np.array(lattice_q), rng.integers(-6, 7, size=(59, 3)) * 0.5,
                         rng.uniform(-3, 3, size=(64, 3))])
    got = g.photon_gather(qs)
    ties = 0
    for q, gv in zip(qs, got):
        ev, straddle = _oracle_irradiance(o, pos, pwr, q, k)
        if straddle:  # the replay: the reference's photons, summed in its poll order
            ties += 1
            assert np.array_equal(gv, ev), (q, gv, ev)
        else:
            np.testing.assert_allclose(gv, ev, rtol=1e-12, atol=0)
    assert ties >= 5


def _tie_plane_scene(tmp_path, k):
    """A photon-mapped quad (z = -4) whose photons sit on a 0.25 lattice in its plane, a quarter of them
    duplicated with other powers: every shading point's neighbourhood boundary falls on a duplicated
    pair at some pixels (equal distances, different powers)."""
    (tmp_path / "tie.cli").write_text(
        f"fov 60\nbackground 0 0 0\npoint_light 0 3 0 1 1 1\ndiffuse_photons 100 {k} 0.6\n"
        "diffuse .6 .6 .6 .1 .1 .1\nbegin quad\nvertex -3 -3 -4\nvertex 3 -3 -4\nvertex 3 3 -4\nvertex -3 3 -4\nend\n")
    rng = np.random.default_rng(k)
    g = np.stack(np.meshgrid(np.arange(-12, 13), np.arange(-12, 13), indexing="ij"), -1).reshape(-1, 2) * 0.25
    g = np.concatenate([g, np.full((len(g), 1), -4.0)], 1)
    pos = np.concatenate([g, g[rng.choice(len(g), len(g) // 4, replace=False)]])
    pos = pos[rng.permutation(len(pos))]
    return pos, rng.random((len(pos), 3)) * 0.01


@pytest.mark.parametrize("k", [4, 9])
def test_render_with_tied_neighbourhoods_matches_oracle(tmp_path, k):
    pos, pwr = _tie_plane_scene(tmp_path, k)
    g = rt.Scene.load_cli("tie.cli", scene_dir=tmp_path, textures={})
    g.set_photons(pos, pwr)
    o = OracleScene(tmp_path, "tie.cli")
    o.set_photons(pos, pwr)
    rg, ag = g.render(64, 64, spp=1, seed=7)
    ro, ao, _ = o.render(64, 64, spp=1, seed=7)
    assert_exact_decisions(compare(rg, ag, ro, ao))


@pytest.mark.parametrize("n", [25, 187, 60000, 262147])
def test_device_kdtree_is_the_references(tmp_path, monkeypatch, n):
    """The kd-tree the tie replay walks, built on the device (photon_build.hip: per-level stable radix
    sorts), is the reference's build_tree node for node: the host restatement (rt_photon_kdtree,
    itself pinned against tests/test_knn_ties.py's Python build_tree) with every photon identified by
    its position and power in the photon map's leaf order. Duplicated lattice points and signed
    zeros make the stable-sort ties decisive; n = 25 is the smallest map built on the device."""
    (tmp_path / "t.cli").write_text("fov 60\nbackground 0 0 0\npoint_light 0 5 0 1 1 1\ndiffuse_photons 100 8 10\n"
                                    "diffuse .5 .5 .5 0 0 0\nsphere 1 0 0 -5\n")
    rng = np.random.default_rng(n)
    pos = rng.integers(-6, 7, size=(n, 3)).astype(np.float64) * 0.5
    pos[rng.random((n, 3)) < 0.1] = -0.0
    pwr = rng.random((n, 3))
    g = rt.Scene.load_cli("t.cli", scene_dir=tmp_path, textures={})
    g.set_photons(pos, pwr)
    dev = g.photon_kdtree()
    _, _, ppos, ppwr = g.photon_map()
    host = rt.photon_kdtree(pos)
    assert np.array_equal(dev[:, 1:], host[:, 1:])
    assert np.array_equal(ppos[dev[:, 0]], pos[host[:, 0]])
    assert np.array_equal(ppwr[dev[:, 0]], pwr[host[:, 0]])


@pytest.mark.parametrize("seed", [3, 4])
def test_gather_ties_at_the_largest_k(tmp_path, seed):
    """k = KNN_MAX = 256, the largest neighbourhood the device takes: PriorityQueue.offer adds before
    poll trims, so the replay's heap holds 257 entries for a moment (its LDS arrays have
    K + 1 slots). A 9 x 9 x 5 lattice with duplicated points puts ties across the 256th distance."""
    k = 256
    cli = tmp_path / "knn.cli"
    cli.write_text(f"fov 60\nbackground 0 0 0\npoint_light 0 5 0 1 1 1\ndiffuse_photons 100 {k} 100\n"
                   "diffuse .5 .5 .5 0 0 0\nsphere 1 0 0 -5\n")
    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), np.arange(-2, 3), indexing="ij"), -1).reshape(-1, 3)
    pos = np.concatenate([grid, grid[rng.choice(len(grid), 150, replace=False)]]).astype(np.float64)
    pos = pos[rng.permutation(len(pos))]
    pwr = rng.random((len(pos), 3))
    g = rt.Scene.load_cli("knn.cli", scene_dir=tmp_path, textures={})
    g.set_photons(pos, pwr)
    o = OracleScene(tmp_path, "knn.cli")
    o.set_photons(pos, pwr)
    qs = np.concatenate([np.array([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.5, 0.5, 0.5), (1.0, -1.0, 0.0)]),
                         rng.integers(-4, 5, size=(28, 3)) * 0.5, rng.uniform(-2, 2, size=(32, 3))])
    got = g.photon_gather(qs)
    ties = 0
    for q, gv in zip(qs, got):
        ev, straddle = _oracle_irradiance(o, pos, pwr, q, k)
        if straddle:
            ties += 1
            assert np.array_equal(gv, ev), (q, gv, ev)
        else:
            np.testing.assert_allclose(gv, ev, rtol=1e-12, atol=0)
    assert ties >= 5


def test_gather_u8_bucket_carry_falls_back(tmp_path):
    """The counting passes keep 128 u8 buckets per lane (KNN_HB); a bucket holding more than 255
    photons carries into its neighbour, which the pass detects from the buckets' sum and repeats with
    u16 buckets. 300 photons at distinct distances within 3e-7 of radius 1 around the query points
    land in one bucket of the first pass: the k = 100 nearest must still be the oracle's."""
    k = 100
    cli = tmp_path / "knn.cli"
    cli.write_text(f"fov 60\nbackground 0 0 0\npoint_light 0 5 0 1 1 1\ndiffuse_photons 100 {k} 100\n"
                   "diffuse .5 .5 .5 0 0 0\nsphere 1 0 0 -5\n")
    rng = np.random.default_rng(11)
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    shell = d * (1.0 + np.arange(300)[:, None] * 1e-9)
    far = rng.normal(size=(60, 3))
    far *= (2.0 + rng.random((60, 1))) / np.linalg.norm(far, axis=1, keepdims=True)
    pos = np.concatenate([shell, far])
    pos = pos[rng.permutation(len(pos))]
    pwr = rng.random((len(pos), 3))
    g = rt.Scene.load_cli("knn.cli", scene_dir=tmp_path, textures={})
    g.set_photons(pos, pwr)
    o = OracleScene(tmp_path, "knn.cli")
    o.set_photons(pos, pwr)
    qs = np.array([(0.0, 0.0, 0.0), (1e-9, 0.0, 0.0), (0.0, -2e-9, 1e-9)])
    got = g.photon_gather(qs)
    for q, gv in zip(qs, got):
        ev, straddle = _oracle_irradiance(o, pos, pwr, q, k)
        assert not straddle
        np.testing.assert_allclose(gv, ev, rtol=1e-12, atol=0)
