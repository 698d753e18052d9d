"""The arithmetic facts behind the render kernel's known normalisations (csrc/trace_device.h: unit_len /
renorm, planar_test's sign test, nrmz_m for the light distance), shown in numpy, which is
IEEE fp64 and unfused like the kernels (-ffp-contract=off).

The model below is the device's: mag sums (x^2 + y^2) + z^2, nrmz divides each component by the rounded square
root and leaves the zero vector alone, renorm re-normalises an unflagged direction, counts the changes in `ver`
and flags the direction once normalising it gives it back."""
import numpy as np
import pytest

N = 200_000
ULP1 = 2.0 ** -52
STEPS = 8


def _s(d):
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _nrmz(d):
    with np.errstate(all="ignore"):
        m = np.sqrt(_s(d))
        return np.where((m == 0)[:, None], d, d / m[:, None]), m


def _unit(d):
    with np.errstate(all="ignore"):
        s = _s(d)
    return (s == 1.0) | (s == 1.0 + ULP1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _renorm_seq(d0, shortcut):
    """(d, ver, stable, moved) after each of STEPS renorm calls, and how many lanes ran the full nrmz per call."""
    d = d0.copy()
    n = len(d)
    ver, stable, moved = np.zeros(n, np.uint32), np.zeros(n, bool), np.zeros(n, bool)
    seq, full = [], []
    for _ in range(STEPS):
        act = ~stable
        if shortcut:
            u = act & _unit(d)
            stable = stable | u
            act = act & ~u
        nd, _ = _nrmz(d)
        eq = (nd == d).all(1)  # veq: NaN and nothing else differs from itself
        stable = stable | (act & eq)
        ch = act & ~eq
        moved = moved | ch
        ver = ver + ch
        d = np.where(act[:, None], nd, d)
        full.append(int(act.sum()))
        seq.append((_bits(d).copy(), ver.copy(), stable.copy(), moved.copy()))
    return seq, full


def _random_dirs(rng):
    v = rng.normal(size=(N, 3))
    return _nrmz(v)[0]  # one normalisation, as a ray constructor leaves it


def _camera_dirs(rng):
    v = np.stack([rng.uniform(-0.5, 0.5, N), rng.uniform(-0.5, 0.5, N), np.full(N, -1.0)], 1)
    return _nrmz(v)[0]


def _edge_dirs():
    big, den, tiny = 1.5e200, 5e-324, 2.2250738585072014e-308
    rows = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1),
            (1, 0.0, -0.0), (-0.0, 1, 0.0), (0.0, -0.0, -1), (0.6, -0.0, 0.8), (0.0, 0.6, -0.8),
            (big, 1, 1), (1, -big, 0), (big, big, big), (np.inf, 0, 0), (1, np.inf, -np.inf),
            (den, 0, 0), (den, den, -den), (tiny, -tiny, 0), (1, den, 0), (3e-160, 4e-160, 0),
            (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0),
            (np.nan, 0, 0), (1, np.nan, 0), (np.nan, np.nan, np.nan),
            (3.7, 0, 0), (0.3, 0.4, 0.5), (1e-3, 1, 1e3)]
    return np.array(rows, dtype=np.float64)


@pytest.fixture(scope="module")
def dirs():
    rng = np.random.default_rng(20260)
    return {"random": _random_dirs(rng), "camera": _camera_dirs(rng), "edge": _edge_dirs()}


def classify(d0, steps=12):
    """Per direction: the number of normalisations after which it is fixed (0..steps), or -2 for a period-2
    cycle, -1 for anything else (NaN, no cycle found)."""
    d, hist = d0.copy(), [_bits(d0).copy()]
    out = np.full(len(d0), -1)
    for k in range(steps):
        d = _nrmz(d)[0]
        hist.append(_bits(d).copy())
    for k in range(steps, -1, -1):
        if k < steps:
            fixed = (hist[k] == hist[k + 1]).all(1)
            out[fixed] = k
    osc = (out == -1) & (hist[steps] == hist[steps - 2]).all(1) & ~(hist[steps] == hist[steps - 1]).all(1)
    out[osc] = -2
    return out


def test_sqrt_is_one_exactly_for_the_two_sums():
    one = np.float64(1.0)
    up1, up2, dn1 = np.nextafter(one, 2), np.nextafter(np.nextafter(one, 2), 2), np.nextafter(one, 0)
    assert up1 == 1.0 + ULP1
    assert np.sqrt(one) == 1.0 and np.sqrt(up1) == 1.0
    assert np.sqrt(up2) != 1.0 and np.sqrt(dn1) != 1.0 and np.sqrt(np.nextafter(dn1, 0)) != 1.0
    # and x / 1.0 is x, signed zeros, denormals, infinities included
    x = np.array([0.0, -0.0, 5e-324, -1.0, 0.1, np.inf, -np.inf, 1.7976931348623157e308])
    assert np.array_equal(_bits(x / np.sqrt(up1)), _bits(x))


@pytest.mark.parametrize("name", ["random", "camera", "edge"])
def test_renorm_sequence_is_the_same_with_the_shortcut(name, dirs):
    d0 = dirs[name]
    want, full_w = _renorm_seq(d0, False)
    got, full_g = _renorm_seq(d0, True)
    for k, (w, g) in enumerate(zip(want, got)):
        for what, a, b in zip(("d", "ver", "stable", "moved"), w, g):
            assert np.array_equal(a, b), (name, "call", k, what, int((a != b).sum()))
    print(name, "lanes running the full normalisation per call: without", full_w, "with", full_g)
    assert sum(full_g) <= sum(full_w)
    if name != "edge":
        assert sum(full_g) < 0.8 * sum(full_w)  # the confirming normalisation of every settling lane is gone


@pytest.mark.parametrize("name", ["random", "camera"])
def test_unit_sum_is_the_fixed_point_condition(name, dirs):
    """nrmz(d) == d exactly when the squared length is 1 or 1 + 2^-52, at every step of the sequence."""
    d = dirs[name]
    for _ in range(4):
        nd, m = _nrmz(d)
        fixed = (_bits(nd) == _bits(d)).all(1)
        assert np.array_equal(fixed, _unit(d)) and np.array_equal(fixed, m == 1.0)
        d = nd


def test_random_set_holds_the_period_two_directions(dirs):
    """Condition on the input: the shortcut is exercised on lanes that never settle (about 0.6 % of random
    directions alternate between two values, one a few ulps short of unit length, the other 2^-52 over)."""
    cls = classify(dirs["random"])
    n_osc = int((cls == -2).sum())
    print("random: fixed after k normalisations", {k: int((cls == k).sum()) for k in range(0, 6)}, "period 2:", n_osc,
          "other:", int((cls == -1).sum()))
    assert n_osc >= 256
    cam = classify(dirs["camera"])
    print("camera: period 2:", int((cam == -2).sum()), "fixed at once", int((cam == 0).sum()))
    d = dirs["random"][cls == -2]
    m1 = _nrmz(d)[1]
    m2 = _nrmz(_nrmz(d)[0])[1]
    print("period-2 magnitudes", np.unique(np.concatenate([m1, m2])).tolist())
    assert (m1 != 1.0).all() and (m2 != 1.0).all()  # just below 1 and just above, in turn
    assert not _unit(d).any()


def test_light_distance_is_the_normalisations_magnitude():
    """(a - b)^2 == (b - a)^2 bit for bit, so |fwd - origin| summed in mag's order is the magnitude that
    normalising (origin - fwd) divides by; a -0 component of the origin, which the identity CTM turns into +0,
    changes neither."""
    rng = np.random.default_rng(7)
    a = rng.normal(size=(N, 3)) * 10.0 ** rng.integers(-3, 4, (N, 1))
    b = rng.normal(size=(N, 3)) * 10.0 ** rng.integers(-3, 4, (N, 1))
    a[:64], b[:64] = b[:64], b[:64].copy()  # coincident points
    a[64:128, 0], b[128:192, 1] = -0.0, 0.0
    with np.errstate(all="ignore"):
        eye = np.eye(3)  # xpt: each row accumulated from +0 in column order, then + 0 * 1
        ident = np.stack([(((0.0 + eye[r, 0] * a[:, 0]) + eye[r, 1] * a[:, 1]) + eye[r, 2] * a[:, 2]) + 0.0 * 1.0
                          for r in range(3)], 1)
        assert np.array_equal(_bits((ident - b) * (ident - b)), _bits((b - a) * (b - a)))
        m = _nrmz(ident - b)[1]
        t = np.sqrt(_s(b - a))
    assert np.array_equal(_bits(m), _bits(t))


def test_planar_sign_test_rejects_what_the_division_rejects():
    """planar_test after orientation: pr < 0. t = -num / pr passes t > 1e-7 only if num > 0, so !(num > 0)
    returns false before the division; every num > 0 still goes through the division as before."""
    rng = np.random.default_rng(11)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-7, -1e-7, 1e-300, -1e-300, 1.0, -1.0, 1e300, -1e300,
                        np.inf, -np.inf, np.nan, 1.7976931348623157e308, -1.7976931348623157e308])
    num = np.concatenate([special.repeat(len(special)), rng.normal(size=N) * 10.0 ** rng.integers(-12, 12, N)])
    prs = -np.abs(special[~np.isnan(special) & (special != 0)])
    pr = np.concatenate([np.tile(special, len(special)), -np.abs(rng.normal(size=N)) * 10.0 ** rng.integers(-12, 12, N)])
    pr[: len(special) ** 2] = np.resize(prs, len(special) ** 2)
    assert (pr < 0).all() and np.isnan(num).any() and (num == 0).any()
    with np.errstate(all="ignore"):
        t = -num / pr
    passes = t > 1e-7
    early = ~(num > 0)
    assert not (passes & early).any()
    assert passes.sum() > N // 4 and early.sum() > N // 4
