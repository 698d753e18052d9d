"""The upload-time hit-normal table's place in the layout (csrc/rt_types.h): 48 B per triangle behind the fp32
edge records, counted by rt_scene_inspect_cli's byte estimate, and nothing per light (the table of light
positions was measured and not built); and the reason the table stores orientation B
instead of negating orientation A."""
import numpy as np

from distraytracer_old_amd import rt
from tests import trace_util as tu

# a top-level triangle costs its TriD, its TriF and its TopD, a light its LightD
TRI_BYTES, LIGHT_BYTES = 128 + 80 + 16, 272
HIT_NRM_BYTES = 2 * 3 * 8


def _text(ntri, nlight):
    L = ["fov 60", "background 0.1 0.1 0.2"] + ["point_light %d 4 0 .8 .8 .8" % k for k in range(nlight)]
    L += ["diffuse .8 .8 .8 .2 .2 .2", "translate 0 0 -3"] + tu._tri_lines(tu.random_tris(ntri, tu.SEED + 9), 1.0)
    return "\n".join(L) + "\n"


def test_library_loads_and_the_estimate_counts_the_table(tmp_path):
    assert rt.lib() is not None and len(rt.build_id()) == 16
    info = {}
    for ntri, nlight in ((7, 1), (8, 1), (300, 1), (7, 3)):
        (tmp_path / f"s_{ntri}_{nlight}.cli").write_text(_text(ntri, nlight))
        info[ntri, nlight] = rt.inspect_cli(f"s_{ntri}_{nlight}.cli", scene_dir=tmp_path, textures={})
        assert info[ntri, nlight]["triangles"] == ntri and info[ntri, nlight]["lights"] == nlight
    base = info[7, 1]["device_bytes"]
    assert info[8, 1]["device_bytes"] - base == TRI_BYTES + HIT_NRM_BYTES
    assert info[300, 1]["device_bytes"] - base == 293 * (TRI_BYTES + HIT_NRM_BYTES)
    assert info[7, 3]["device_bytes"] - base == 2 * LIGHT_BYTES


def _nrmz(v):
    """trace_device.h nrmz: (x^2 + y^2) + z^2, a square root, three divisions; the zero vector stays."""
    m = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]
    with np.errstate(all="ignore"):
        return np.where(m == 0, v, v / m)


def _xvec(m, v):
    """trace_device.h xvec: each row summed from +0.0 in column order, the fourth column times 0.0."""
    r = np.zeros_like(v)
    for row in range(3):
        a = np.zeros(len(v))
        for c in range(3):
            a = a + m[:, row, c] * v[:, c]
        r[:, row] = a + m[:, row, 3] * 0.0
    return r


def test_orientation_b_is_not_the_negated_orientation_a():
    """h.nrm = nrmz(xvec(adj, nrmz(+-n))). xvec sums from +0.0, so a component that is exactly zero is +0 for
    both orientations: on normals and adjoints with zero entries -A has a -0 where B has +0. The table
    therefore holds both orientations. (0.0 - A equals B on all of these cases, which is an observation and
    no proof: the kernels do not rely on it.)"""
    g = np.random.default_rng(tu.SEED + 10)
    n = 20000
    nrm = g.normal(size=(n, 3)) * (g.random((n, 3)) < 0.5)
    adj = g.normal(size=(n, 3, 4)) * (g.random((n, 3, 4)) < 0.6)
    a = _nrmz(_xvec(adj, _nrmz(nrm)))
    b = _nrmz(_xvec(adj, _nrmz(-nrm)))
    assert np.array_equal(b, -a)  # equal as numbers
    differ = (b.view(np.uint64) != (-a).view(np.uint64)).any(1)
    print("B != -A bitwise in", int(differ.sum()), "of", n)
    assert differ.sum() >= 1000
    assert ((a == 0) | (b.view(np.uint64) == (-a).view(np.uint64))).all()  # only the sign of a zero differs
    assert np.array_equal((0.0 - a).view(np.uint64), b.view(np.uint64))
