"""The photon gather (irradiance<> in csrc/trace_kernels.h: knn_hist_pass, photon_scan, photon_scan_pk,
knn_java_) against the oracle's find_near over its whole branch space, and the photon BVH against an
independent numpy builder. tests/knn_util.py holds the fixtures; tests/test_knn_space.py proves on
the CPU that each fixture reaches the branch it is named for (the reach floors) and that brute force
agrees with the oracle on all of them.

Tolerance: where photons at the k-th distance are both in and out of the set (straddle) the lane
replays find_near and sums in its poll order: bit-equal. Elsewhere the powers are summed in scan
order, the oracle's in poll order: 1e-12 relative, atol 0 (the project's gather tolerance; the sum's
own bound is (k + 3) 2^-52, under 6e-14 at k = 256). Non-finite values (a k-th distance of 0) equal;
no photon within max_dist: exactly 0. The worst deviation per case is printed."""
import numpy as np
import pytest

from distraytracer_old_amd import rt
from oracle.oracle import OracleScene
from tests import knn_util as ku
from tests.parity import assert_exact_decisions, compare

pytestmark = pytest.mark.gpu

F_C5 = 1 | 8 | 4 | 32  # FT_PRIM | FT_TRANS | FT_PHOTON | FT_LIGHTX: the variant compiled in render_minreg.hip


def _scene(tmp_path, k, md, pos, pwr, text=ku.scene_text):
    (tmp_path / "knn.cli").write_text(text(k, md))
    g = rt.Scene.load_cli("knn.cli", scene_dir=tmp_path, textures={})
    g.set_photons(pos, pwr)
    return g


def _grid1000():
    """Heavy coordinate ties and signed zeros (as test_gpu_photon_map_build_ties_and_sizes makes)."""
    rng = np.random.default_rng(1000)
    pos = rng.integers(-3, 4, size=(1000, 3)).astype(np.float64) * 0.25
    pos[rng.random((1000, 3)) < 0.2] = -0.0
    return pos, rng.random((1000, 3))


@pytest.mark.parametrize("build", ["device", "host"])
@pytest.mark.parametrize("name", ku.FEW + ("plane", "cluster", "dup", "grid1000"))
def test_photon_map_is_the_numpy_builders(tmp_path, monkeypatch, name, build):
    """Both product builders (photon_build.hip, the default above one leaf; photon.cpp) against the
    independent restatement: node for node, leaf order included."""
    if name == "grid1000":
        pos, pwr = _grid1000()
        want = ku.numpy_photon_map(pos, pwr)
    else:
        fx = ku.fixture(name)
        pos, pwr = fx["pos"], fx["pwr"]
        want = ku.photon_map_of(name)
    if build == "host":
        monkeypatch.setenv("DISTRAYTRACER_PHOTON_BUILD", "host")
    g = _scene(tmp_path, 8, 10., pos, pwr)
    got = g.photon_map()
    g.close()
    assert got[0].shape == want[0].shape and got[1] == want[1]
    assert rt.photon_maps_equal(got, want)


def _assert_gather(got, name, k, md):
    irr, straddle, sets = ku.oracle_reference(name, k, md)
    worst = 0.0
    for j, (gv, ev) in enumerate(zip(got, irr)):
        fin = np.isfinite(ev)
        if len(sets[j]) == 0:
            assert np.array_equal(gv, np.zeros(3)) and not np.signbit(gv).any(), (j, gv)
        elif straddle[j] or not fin.all():
            assert np.array_equal(gv, ev, equal_nan=True), (j, gv, ev)
        else:
            nz = ev != 0
            if nz.any():
                worst = max(worst, float((np.abs(gv[nz] - ev[nz]) / np.abs(ev[nz])).max()))
            np.testing.assert_allclose(gv, ev, rtol=1e-12, atol=0, err_msg=f"query {j}")
    return worst


@pytest.mark.parametrize("name,k,md", ku.CASES, ids=ku.CASE_IDS)
def test_gather_matches_oracle(tmp_path, name, k, md):
    fx = ku.fixture(name)
    g = _scene(tmp_path, k, md, fx["pos"], fx["pwr"])
    got = g.photon_gather(fx["q"])
    g.close()
    worst = _assert_gather(got, name, k, md)
    _, straddle, sets = ku.oracle_reference(name, k, md)
    print(f"\nknn-space {name} k={k} max_dist={md:g}: worst relative deviation {worst:.2e} "
          f"({int(straddle.sum())} straddles, {sum(len(s) == 0 for s in sets)} empty, of {len(sets)})")


def _cluster_orders():
    q = ku.fixture("cluster")["q"]
    n = len(q)
    near, uni = np.arange(64), np.arange(64, 192)
    inter = np.empty(128, dtype=np.int64)
    inter[0::2], inter[1::2] = uni[:64], near  # a wave's first lane is a sparse-region point
    octant = (q[:, 0] > 0) * 4 + (q[:, 1] > 0) * 2 + (q[:, 2] > 0)
    return {"generated": np.arange(n),
            "region": np.lexsort((np.linalg.norm(q, axis=1), octant)),  # by octant of space, then radius
            "interleaved": np.concatenate([inter, uni[64:], np.arange(192, n)]),
            "permuted": np.random.default_rng(7).permutation(n)}


@pytest.mark.parametrize("k,md", ku.PARAMS["cluster"])
def test_gather_is_independent_of_wave_mates(tmp_path, k, md):
    """A lane's result does not depend on the other 63 lanes of its gather call: not on whether the
    wave scans as one packet or lane by lane (lw, decided by where the others lie), not on which
    photons the packet's union brings past it, not on the histogram path another lane's window
    forces. Rank, pixel-list and adaptive renders promise frames bit-equal to rt_render on it."""
    fx = ku.fixture("cluster")
    q = fx["q"]
    g = _scene(tmp_path, k, md, fx["pos"], fx["pwr"])
    raw, root, _, _ = g.photon_map()
    nodes = ku.as_nodes(raw)
    R2max = ku.max_dist2(md)
    results, lanewise, packet = {}, 0, 0
    for name, order in _cluster_orders().items():
        assert sorted(order.tolist()) == list(range(len(q)))
        out = np.empty_like(q)
        out[order] = g.photon_gather(q[order])
        results[name] = out
        for w in range(0, len(q), 64):
            pts = q[order[w:w + 64]]
            lw = ku.wave_lanewise(pts, ku.start_window(nodes, root, pts[0], k, R2max)[0])
            lanewise += lw
            packet += not lw
    assert lanewise >= 2 and packet >= 2, (lanewise, packet)
    base = results["generated"]
    for name, out in results.items():
        assert np.array_equal(out.view(np.uint64), base.view(np.uint64)), name
    for n in (1, 63, 64, 65):
        assert np.array_equal(g.photon_gather(q[:n]).view(np.uint64), base[:n].view(np.uint64)), n
    g.close()
    _assert_gather(base, "cluster", k, md)


@pytest.mark.parametrize("k,md", [(50, 10.), (256, 10.)])
def test_histogram_width_knob_changes_nothing(tmp_path, monkeypatch, k, md):
    """DISTRAYTRACER_KNN_U16_MAX=100 sends every pass over more than 100 photons through the u16 and
    then the u32 counters (the model: at least 32 of the cluster's queries): same doubles. The wider
    counters count on the u8 pass's own 128-bucket grid (knn_hist_window), so a lane ends on the same
    final window and sums its photons in the same order. (With whole-window 64- and 16-bucket passes
    the k-sets were the same but 69 of 768 doubles at k = 50 and 190 of 768 at k = 256 differed by up
    to 4 ulp: the sum's order followed the final window.)"""
    fx = ku.fixture("cluster")
    g = _scene(tmp_path, k, md, fx["pos"], fx["pwr"])
    base = g.photon_gather(fx["q"])
    g.close()
    monkeypatch.setenv("DISTRAYTRACER_KNN_U16_MAX", "100")
    h = _scene(tmp_path, k, md, fx["pos"], fx["pwr"])
    low = h.photon_gather(fx["q"])
    h.close()
    assert sum(e["u32"] for e in ku.model_events("cluster", k, md, u16max=100)) >= 32
    worst = _assert_gather(low, "cluster", k, md)  # the same k-sets: the oracle's, within the gather's tolerance
    ulps = np.abs(low.view(np.int64) - base.view(np.int64))
    print(f"\nknn-space knob k={k}: {int((ulps != 0).sum())} of {ulps.size} doubles differ from the default's, by at most "
          f"{int(ulps.max())} ulp; worst relative deviation from the oracle {worst:.2e}")
    assert np.array_equal(low.view(np.uint64), base.view(np.uint64))


@pytest.mark.parametrize("k", [9, 50])
def test_render_kernels_gather_matches_oracle(tmp_path, k):
    """The render kernel's own copy of the gather (the C5 variant, another translation unit under other
    compiler flags than rt_photon_gather's): a plane whose photons hold a 1,500-photon clump of
    radius 1e-3 and a point repeated 40 times, every pixel's decisions the oracle's."""
    pos, pwr = ku.plane_render_photons()
    g = _scene(tmp_path, k, 0.6, pos, pwr, text=ku.plane_scene_text)
    assert g.variant()[0] == F_C5
    o = OracleScene(tmp_path, "knn.cli")
    o.set_photons(pos, pwr)
    rg, ag = g.render(32, 32, spp=1, seed=7)
    ro, ao, _ = o.render(32, 32, spp=1, seed=7)
    g.close()
    assert_exact_decisions(compare(rg, ag, ro, ao))
