"""The denoiser's filter (include/distraytracer.h, "Denoising an accumulated frame") restated in numpy: the init,
one level and the output, vectorised over pixels with a loop over taps. Every step is one IEEE fp64 operation in
the header's order, so the results are compared with the device's by byte equality. A helper, not a test.

Planes are float64 c [H, W, 3] and v [H, W]; n is the per-pixel sample count int [H, W]; the guides are the dict
Denoiser.guides() returns (float32 normal / pos / depth, int32 material)."""
import numpy as np

EPS = 1e-10
H5 = {-2: 0.0625, -1: 0.25, 0: 0.375, 1: 0.25, 2: 0.0625}
B3 = {-1: 0.25, 0: 0.5, 1: 0.25}


def clamp1(c):
    """min(1, c), a NaN stays"""
    return np.where(1.0 <= c, 1.0, c)


def init(sum_, sq, n):
    """(c, v) from Accumulator.state()'s sums and the counts"""
    n = np.asarray(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        dn = n.astype(np.float64)
        dn1 = (n - 1).astype(np.float64)
        c = np.where((n >= 1)[..., None], clamp1(sum_ / dn[..., None]), 0.0)
        e = None
        for k in range(3):
            m = sum_[..., k] / dn
            mm = m * m
            v = sq[..., k] / dn - mm
            v = np.where(v < 0, 0.0, v)
            ec = ((v * dn) / dn1) / dn
            e = ec if k == 0 else np.where(ec > e, ec, e)
        v = np.where(n >= 2, e, 1.0)
    return c, v


def level(c, v, n, guides, stride, normal_log2, sigma_l, sigma_z):
    """one a-trous level at tap stride `stride` -> (c', v')"""
    H, W = v.shape
    n = np.asarray(n)
    live = n > 0
    mat = guides["material"]
    nrm = guides["normal"].astype(np.float64)
    pos = guides["pos"].astype(np.float64)
    depth = guides["depth"].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        g = np.zeros((H, W))
        for dy in (-1, 0, 1):
            yy = np.clip(ys + dy, 0, H - 1)
            for dx in (-1, 0, 1):
                xx = np.clip(xs + dx, 0, W - 1)
                g = g + (B3[dy] * B3[dx]) * v[yy, xx]
        dp = sigma_l * np.sqrt(g) + EPS
        zden = sigma_z * depth + EPS
        S = np.zeros((H, W))
        C = np.zeros((H, W, 3))
        V = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * stride, xs + dx * stride
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                cq, vq = c[qyc, qxc], v[qyc, qxc]
                if dy == 0 and dx == 0:
                    take = inside
                    w = np.ones((H, W))
                else:
                    take = inside & live[qyc, qxc] & (mat[qyc, qxc] == mat)
                    nq, pq = nrm[qyc, qxc], pos[qyc, qxc]
                    t = ((nrm[..., 0] * nq[..., 0]) + (nrm[..., 1] * nq[..., 1])) + (nrm[..., 2] * nq[..., 2])
                    wn = np.where(t > 0, t, 0.0)
                    for _ in range(normal_log2):
                        wn = wn * wn
                    e = pq - pos
                    r = np.abs(((nrm[..., 0] * e[..., 0]) + (nrm[..., 1] * e[..., 1])) + (nrm[..., 2] * e[..., 2])) / zden
                    uz = 1.0 + r * r
                    miss = mat == -1
                    wn = np.where(miss, 1.0, wn)
                    uz = np.where(miss, 1.0, uz)
                    a = np.abs(c - cq)
                    m = a[..., 0]
                    m = np.where(a[..., 1] > m, a[..., 1], m)
                    m = np.where(a[..., 2] > m, a[..., 2], m)
                    r = m / dp
                    ul = 1.0 + r * r
                    w = wn / ((uz * uz) * (ul * ul))
                k = (H5[dy] * H5[dx]) * w
                S = np.where(take, S + k, S)
                C = np.where(take[..., None], C + k[..., None] * cq, C)
                V = np.where(take, V + (k * k) * vq, V)
        c2 = C / S[..., None]
        v2 = V / (S * S)
    return np.where(live[..., None], c2, c), np.where(live, v2, v)


def output(c):
    """(rgb float32, argb int32) of the final colour plane"""
    cc = clamp1(c)
    rgb = cc.astype(np.float32)
    with np.errstate(all="ignore"):
        q = np.where(np.isnan(cc), 0.0, np.trunc(cc * 255))
    q = np.clip(q, -2147483648.0, 2147483647.0).astype(np.int64) & 0xFFFFFFFF
    argb = ((255 << 24) + (q[..., 0] << 16) + (q[..., 1] << 8) + q[..., 2]) & 0xFFFFFFFF
    return rgb, argb.astype(np.uint32).view(np.int32)


def run(sum_, sq, n, guides, levels, normal_log2, sigma_l, sigma_z):
    """the planes after `levels` levels -> (c, v)"""
    c, v = init(sum_, sq, n)
    for i in range(levels):
        c, v = level(c, v, n, guides, 1 << i, normal_log2, sigma_l, sigma_z)
    return c, v
