"""The numpy restatement of the denoiser's filter (tests/denoise_ref.py) on its own, on synthetic planes and
guides: the properties the definition promises, which the GPU tests then inherit by byte equality."""
import numpy as np
import pytest

from tests import denoise_ref as ref

H, W = 9, 14
PARAMS = dict(normal_log2=7, sigma_l=4.0, sigma_z=0.01)


def _guides(material=None, seed=1):
    """a tilted plane seen from the origin, one material unless given"""
    r = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    pos = np.stack([xs * 0.1, ys * 0.1, 5 + xs * 0.02], -1).astype(np.float32)
    nrm = np.broadcast_to(np.array([-0.19611613, 0.0, 0.98058068], dtype=np.float32), (H, W, 3)).copy()
    nrm += (r.random((H, W, 3)) * 1e-3).astype(np.float32)
    depth = np.sqrt((pos.astype(np.float64) ** 2).sum(-1)).astype(np.float32)
    mat = np.zeros((H, W), dtype=np.int32) if material is None else np.asarray(material, dtype=np.int32)
    return {"normal": nrm, "pos": pos, "depth": depth, "material": mat}


def _noisy(seed=2):
    r = np.random.default_rng(seed)
    c = r.random((H, W, 3))
    v = r.random((H, W)) * 0.01
    return c, v


def _levels(c, v, n, g, levels):
    for i in range(levels):
        c, v = ref.level(c, v, n, g, 1 << i, **PARAMS)
    return c, v


def test_the_tap_weights_sum_to_one():
    h = [ref.H5[i] for i in range(-2, 3)]
    assert sum(a * b for a in h for b in h) == 1.0
    b = [ref.B3[i] for i in range(-1, 2)]
    assert sum(a * c for a in b for c in b) == 1.0
    assert ref.H5[0] * ref.H5[0] == 9 / 64  # the centre tap: S's lower bound


def test_a_constant_image_is_a_fixed_point():
    # 0.375 and the plane's weights are dyadic, so even the rounding leaves the colour where it is up to the
    # last place; the assertion allows one rounding per tap and level
    c = np.full((H, W, 3), 0.375)
    v = np.full((H, W), 0.25)
    n = np.full((H, W), 4)
    c5, v5 = _levels(c, v, n, _guides(), 5)
    assert np.abs(c5 - c).max() <= 25 * 5 * 2.0 ** -53
    assert (v5 > 0).all() and (v5 <= v).all()  # averaging certain neighbours never raises the variance


def test_zero_levels_is_the_identity():
    r = np.random.default_rng(3)
    n = r.integers(1, 6, (H, W))
    s = r.random((H, W, 3)) * n[..., None]
    q = s * s + r.random((H, W, 3))
    c0, v0 = ref.init(s, q, n)
    c, v = ref.run(s, q, n, _guides(), 0, **PARAMS)
    assert np.array_equal(c, c0) and np.array_equal(v, v0)
    assert np.array_equal(c, np.minimum(1.0, s / n[..., None]))  # rt_accum_resolve's double
    assert (v[n == 1] == 1.0).all() and (v[n >= 2] >= 0).all()


def test_no_colour_crosses_a_material_boundary():
    mat = np.zeros((H, W), dtype=np.int32)
    mat[:, W // 2:] = 1
    mat[0:3, 0:3] = -1  # misses are a surface of their own
    c = np.zeros((H, W, 3))
    c[mat == 1] = 1.0
    c[mat == -1] = 0.5
    v = np.full((H, W), 10.0)  # so noisy that the colour edge-stop is open
    n = np.full((H, W), 4)
    c5, _ = _levels(c, v, n, _guides(mat), 5)
    assert (c5[mat == 0] == 0.0).all() and (c5[mat == 1] == 1.0).all() and (c5[mat == -1] == 0.5).all()
    # the same noise inside one material does mix
    c, v = _noisy()
    c1, _ = _levels(c, np.full((H, W), 10.0), n, _guides(), 1)
    assert not np.array_equal(c1, c)


def test_pixels_without_samples_neither_change_nor_leak():
    c, v = _noisy()
    n = np.full((H, W), 4)
    hole = np.zeros((H, W), dtype=bool)
    hole[2, 3] = hole[5, 9] = hole[5, 10] = True
    n[hole] = 0
    c[hole] = 0.0
    v[hole] = 1.0
    g = _guides()
    big = np.full((H, W), 10.0)
    big[hole] = 1.0
    c5, v5 = _levels(c, big, n, g, 5)
    assert (c5[hole] == 0.0).all() and (v5[hole] == 1.0).all()
    # whatever stands in a hole's colour record reaches no other pixel
    c_alt = c.copy()
    c_alt[hole] = 1e6
    c5b, v5b = _levels(c_alt, big, n, g, 5)
    assert np.array_equal(c5b[~hole], c5[~hole]) and np.array_equal(v5b[~hole], v5[~hole])
    rgb, argb = ref.output(c5)
    assert (rgb[hole] == 0).all() and (argb[hole].view(np.uint32) == 0xFF000000).all()


def test_output_packs_as_the_frame_does():
    c = np.array([[[0.0, 0.5, 1.0], [1.5, 0.999, 0.25]]])
    rgb, argb = ref.output(c)
    assert rgb.dtype == np.float32 and argb.dtype == np.int32
    assert np.array_equal(rgb, np.array([[[0, 0.5, 1], [1, 0.999, 0.25]]], dtype=np.float32))
    assert argb.view(np.uint32).tolist() == [[0xFF007FFF, 0xFFFFFE3F]]
