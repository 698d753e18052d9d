"""The render kernel's average over n = 2^k samples multiplies by 2^-k instead of dividing by n.

x / n and x * 2^-k are the same real number rounded once (2^-k is exact and the product of a
double with a power of two is exact before rounding), so they are the same double for every x:
normal, subnormal (where both round the same shifted significand), zero, infinite and NaN. For an n
that is no power of two 1.0 / n is itself rounded, the product rounds twice, and the results
differ for some x: there the kernel keeps the division.
"""
import numpy as np
import pytest

N_RANDOM = 1 << 21


def doubles():
    """A few million doubles of every class: random bit patterns (every exponent, so subnormals,
    infinities and NaN payloads of both kinds and signs), colour-sized values, and the edge cases."""
    rng = np.random.default_rng(0x5EED)
    bits = rng.integers(0, 1 << 64, size=N_RANDOM, dtype=np.uint64)
    sub = rng.integers(0, 1 << 52, size=N_RANDOM // 4, dtype=np.uint64)  # exponent field 0: subnormals
    sub[::2] |= np.uint64(1 << 63)
    top = (np.uint64(0x7FE) << np.uint64(52)) | rng.integers(0, 1 << 52, size=N_RANDOM // 4, dtype=np.uint64)  # near the largest
    near_sub = (rng.integers(1, 64, size=N_RANDOM // 4, dtype=np.uint64) << np.uint64(52)) | \
        rng.integers(0, 1 << 52, size=N_RANDOM // 4, dtype=np.uint64)  # quotients that round into the subnormals
    sums = rng.random(N_RANDOM) * 130.0  # what the kernel divides: sums of up to spp colours in [0, 1]
    mx, tiny = np.finfo(np.float64).max, np.float64(5e-324)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, mx, -mx, np.nextafter(mx, 0), tiny, -tiny, 3 * tiny,
                     np.finfo(np.float64).tiny, np.nextafter(np.finfo(np.float64).tiny, 0), 1.0, -1.0])
    nan = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001,
                    0x7FF8DEADBEEF0001, 0x7FF4000000000000, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64)
    return np.concatenate([bits.view(np.float64), sub.view(np.float64), top.view(np.float64),
                           near_sub.view(np.float64), sums, edge, nan.view(np.float64)])


X = doubles()


def same_bits(a, b):
    """Bitwise equal: signed zeros, subnormals, infinities, and a NaN operand's payload (quieted the
    same way by both forms)."""
    return a.view(np.uint64) == b.view(np.uint64)


def test_inputs_cover_every_class():
    assert len(X) > 3_000_000
    e = (X.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)
    frac = X.view(np.uint64) & np.uint64((1 << 52) - 1)
    assert ((e == 0) & (frac != 0)).sum() > 100_000  # subnormals
    assert np.isnan(X).sum() > 100 and np.isinf(X).sum() >= 2
    assert (X == np.finfo(np.float64).max).any() and (np.signbit(X) & (X == 0)).any()


@pytest.mark.parametrize("n", [2, 4, 8, 16, 32, 64, 128, 1024])
def test_power_of_two_product_equals_division(n):
    k = n.bit_length() - 1
    inv = np.array([(1023 - k) << 52], dtype=np.uint64).view(np.float64)[0]  # 2^-k from its exponent field, as the kernel
    assert inv == 1.0 / n
    with np.errstate(all="ignore"):
        q, p = X / np.float64(n), X * inv
    ok = same_bits(q, p)
    assert ok.all(), (n, X[~ok][:4], q[~ok][:4], p[~ok][:4])


@pytest.mark.parametrize("n", [3, 5, 70])
def test_other_n_keep_the_division(n):
    with np.errstate(all="ignore"):
        q, p = X / np.float64(n), X * (1.0 / np.float64(n))
    diff = ~same_bits(q, p)
    assert diff.sum() > 1000, (n, int(diff.sum()))  # observed: the product is wrong for a large share of x
