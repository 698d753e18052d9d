"""The photon gather's branch space, CPU side (tests/knn_util.py has the fixtures and what each part
is): brute force against the oracle's find_near on every fixture the GPU test (test_gpu_knn_space.py)
gathers on, and the REACH FLOORS -- the proof that those fixtures take the branches they are named
for, by the numpy photon map and the model of irradiance<>'s bracket loop. A fixture that stops
reaching its branch fails here, on any machine, instead of quietly testing less on the GPU.

Tolerance of the oracle against brute force: (k + 3) 2^-52 relative. Powers are non-negative, so a
k-term sum in any order is within (k - 1) 2^-53 of the exact sum; the area and the division round
once each; the whole doubled. Non-finite values (a k-th distance of exactly 0) must be equal."""
import numpy as np
import pytest

from tests import knn_util as ku


@pytest.mark.parametrize("name,k,md", ku.CASES, ids=ku.CASE_IDS)
def test_brute_force_agrees_with_the_oracle(name, k, md):
    fx = ku.fixture(name)
    o_irr, o_straddle, o_sets = ku.oracle_reference(name, k, md)
    worst = 0.0
    for j, q in enumerate(fx["q"]):
        b_irr, sel, straddle = ku.brute_force(fx["pos"], fx["pwr"], q, k, md)
        idx = o_sets[j]
        assert len(idx) == len(sel), (j, len(idx), len(sel))
        assert straddle == bool(o_straddle[j]), j
        if not straddle:
            assert set(idx.tolist()) == set(sel.tolist()), j
        fin = np.isfinite(b_irr)
        assert np.array_equal(o_irr[j][~fin], b_irr[~fin], equal_nan=True), (j, o_irr[j], b_irr)
        if not straddle and fin.any():
            dev = np.abs(o_irr[j][fin] - b_irr[fin])
            assert np.all(dev <= (k + 3) * 2.0 ** -52 * np.abs(b_irr[fin])), (j, o_irr[j], b_irr)
            nz = b_irr[fin] != 0
            if nz.any():
                worst = max(worst, float((dev[nz] / np.abs(b_irr[fin][nz])).max()))
    print(f"{name} k={k} max_dist={md:g}: oracle vs brute force, worst relative {worst:.2e}")


def _count(name, k, md, pred, **kw):
    return sum(bool(pred(e)) for e in ku.model_events(name, k, md, **kw))


def _widened(e):
    return e["widen_ext"] or e["widen_far"] or e["widen_max"]


def test_reach_plane():
    assert _count("plane", 10, .5, _widened) >= 50          # 122 of 256 measured
    assert _count("plane", 50, .05, lambda e: e["all"]) >= 128  # 256


def test_reach_cluster():
    assert _count("cluster", 256, 10., lambda e: e["u16"]) >= 120        # 247 of 256
    assert _count("cluster", 256, 10., lambda e: e["passes"] >= 4) >= 80  # 120
    assert _count("cluster", 50, 10., lambda e: e["widen_ext"]) >= 40     # 88


@pytest.mark.parametrize("k,md", ku.PARAMS["shell"])
def test_reach_shell_walks_the_edges(k, md):
    assert _count("shell", k, md, lambda e: e["narrow"]) >= 32  # 64 of 64


@pytest.mark.parametrize("k,md", ku.PARAMS["big"])
def test_reach_big_counts_in_u32(k, md):
    assert _count("big", k, md, lambda e: e["u32"]) >= 12  # 26 of 64


def test_reach_dup():
    assert _count("dup", 20, 100., lambda e: e["levels_out"] or e["collapsed"]) >= 8  # 22 of 64
    assert _count("dup", 20, 100., lambda e: e["shell_overflow"]) >= 8                # 22
    # the query on the repeated point: a start window [0, 0) under a far corner at distance 0
    assert ku.model_events("dup", 20, 100.)[-1]["widen_max"]


@pytest.mark.parametrize("k,md", ku.PARAMS["edges"])
def test_reach_edges_puts_photons_on_bucket_edges(k, md):
    """Every query of `edges` has photons whose d2 EQUALS a bucket edge in a pass that settles the
    bucket with one compare (d2 < edge): the case an off-by-one in that compare gets wrong. No other
    fixture reaches it (measured: 0 queries; random coordinates do not land on an edge)."""
    assert _count("edges", k, md, lambda e: e["on_edge"]) == 16


def test_reach_widen_exits_over_all_fixtures():
    far = sum(_count(n, k, md, lambda e: e["widen_far"]) for n, k, md in ku.CASES)
    mx = sum(_count(n, k, md, lambda e: e["widen_max"]) for n, k, md in ku.CASES)
    assert far >= 20  # 983
    assert mx >= 1    # 2: dup's query on the repeated point, at both k


def test_reach_u16_knob_forces_u32():
    """DISTRAYTRACER_KNN_U16_MAX=100 (the GPU test's knob case) sends the cluster's passes to u32."""
    for k, md in ((50, 10.), (256, 10.)):
        assert _count("cluster", k, md, lambda e: e["u32"], u16max=100) >= 32
        assert _count("cluster", k, md, lambda e: e["u32"]) == 0


@pytest.mark.parametrize("name", ["plane", "cluster", "shell", "dup", "few1", "few25", "few30", "plane_small"])
def test_far_corner_bounds_its_node(name):
    """R2far as the model (and the kernel) forms it is a bound: every photon of the node it was taken
    from has d2 <= R2far, so a window widened to it holds K photons."""
    fx = ku.fixture(name)
    raw, root, ppos, _ = ku.photon_map_of(name)
    nodes = ku.as_nodes(raw)
    checked = 0
    for k, _ in ku.PARAMS[name]:
        for q in fx["q"]:
            nd = nodes[ku.start_node(nodes, root, q, k)]
            _, R2far = ku.start_window(nodes, root, q, k, np.inf)  # the corner itself, not capped by max_dist
            if nd["padR"][1] < k:
                continue  # no far corner taken: the window may go to max_dist^2 at once
            first, cnt = int(nd["pad"][0]), int(nd["padR"][1])
            d2 = ku.find_near_d2(ppos[first:first + cnt], q)
            assert d2.max() <= R2far, (k, q)
            checked += 1
    assert checked > 0


def test_numpy_photon_map_shape():
    """The restated map's own invariants (its equality with both product builders is the GPU test's):
    every photon in exactly one leaf, boxes that hold their photons, pre-order numbering."""
    for name in ("few1", "few24", "few25", "cluster"):
        fx = ku.fixture(name)
        raw, root, ppos, ppwr = ku.photon_map_of(name)
        nodes = ku.as_nodes(raw)
        n = len(fx["pos"])
        assert root == 0 and nodes["padR"][0][1] == n and nodes["padR"][0][2] == len(nodes)
        assert sorted(map(tuple, ppos.tolist())) == sorted(map(tuple, fx["pos"].tolist()))
        seen = np.zeros(n, dtype=int)
        for i, nd in enumerate(nodes):
            for ref, first, cnt, mn, mx in ((nd["left"], nd["pad"][0], nd["pad"][1], nd["lmin"], nd["lmax"]),
                                            (nd["right"], nd["pad"][2], nd["padR"][0], nd["rmin"], nd["rmax"])):
                p = ppos[first:first + cnt]
                if cnt:
                    assert np.array_equal(p.min(0), mn) and np.array_equal(p.max(0), mx)
                else:
                    assert np.all(mn == 1e300) and np.all(mx == -1e300)
                if ref < 0:
                    assert cnt <= ku.PHOTON_LEAF
                    seen[first:first + cnt] += 1
                else:
                    assert ref > i and cnt > ku.PHOTON_LEAF and nodes["padR"][ref][1] == cnt
        assert np.all(seen == 1)
        if n <= ku.PHOTON_LEAF:
            assert len(nodes) == 1 and nodes["left"][0] == -1 and nodes["right"][0] == -1 and nodes["padR"][0][0] == 0
