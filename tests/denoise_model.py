"""The denoising filter of DESIGN.md §11 in numpy float32 -- TEST INFRASTRUCTURE ONLY.

Written from the filter's definition (not from csrc/pt_denoise.h): every operation a separately
rounded binary32 operation, a pixel's taps in the fixed order dy outer, dx inner.  The arrays
hold every pixel's running sums; a tap that the definition skips leaves them as they are
(np.where), so the order of the additions per pixel is the definition's.
"""
import numpy as np

f32 = np.float32

DEFAULTS = dict(iterations=5, guide_frames=4, sigma_lum=8.0, sigma_normal=0.1, sigma_albedo=0.1, sigma_depth=0.05)
H5 = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
G3 = [f32(1 / 4), f32(1 / 2), f32(1 / 4)]


def k_of(sigma):
    s = f32(sigma)
    return f32(1.0) / (s * s) if s > 0 else f32(0.0)


def luminance(c):
    return (c[..., 0] * f32(0.2126) + c[..., 1] * f32(0.7152)) + c[..., 2] * f32(0.0722)


def variance_of(moments, n):
    """v of the mean luminance from (..., 2) moments; n an int or an integer array per pixel (>= 2)."""
    with np.errstate(all="ignore"):
        n = np.asarray(n)
        nf = n.astype(f32)
        m = moments[..., 0] / nf
        d = moments[..., 1] / nf - m * m
        d = np.where(d < 0, f32(0), d)
        return (d / (n - 1).astype(f32)).astype(f32)


def pixel_counts(tile_frames, w, h, tw=8, th=8):
    """Per-pixel frame counts from the (tiles_y, tiles_x) counts of tw x th tiles."""
    return np.repeat(np.repeat(np.asarray(tile_frames).astype(np.int64), th, 0), tw, 1)[:h, :w]


def footprint_mask(w, h, ref_dispatch):
    m = np.ones((h, w), bool)
    if ref_dispatch:
        m[:, (w // 10) * 10:] = False
        m[(h // 10) * 10:, :] = False
    return m


def shifted(a, ox, oy, fill):
    """b[y, x] = a[y + oy, x + ox], `fill` where that lies outside the image."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys0, ys1 = max(0, -oy), min(h, h - oy)
    xs0, xs1 = max(0, -ox), min(w, w - ox)
    if ys0 < ys1 and xs0 < xs1:
        b[ys0:ys1, xs0:xs1] = a[ys0 + oy:ys1 + oy, xs0 + ox:xs1 + ox]
    return b


def denoise(image, variance, guides, footprint=None, **params):
    """image (H, W, 4), variance (H, W) or None (unguided), guides (H, W, 8) = N.rgb, Z, A.rgb, 0,
    footprint (H, W) bool or None -> (H, W, 4): rgb filtered, alpha the image's."""
    p = dict(DEFAULTS, **params)
    image = np.asarray(image, f32)
    guides = np.asarray(guides, f32)
    h, w = image.shape[:2]
    fp = np.ones((h, w), bool) if footprint is None else np.asarray(footprint).astype(bool)
    guided = variance is not None
    c = image[..., :3].copy()
    v = np.asarray(variance, f32).copy() if guided else np.zeros((h, w), f32)
    N, Z, A = guides[..., 0:3], guides[..., 3], guides[..., 4:7]
    kl, kn, ka, kz = (k_of(p[s]) for s in ("sigma_lum", "sigma_normal", "sigma_albedo", "sigma_depth"))
    one = f32(1.0)
    with np.errstate(all="ignore"):
        for it in range(p["iterations"]):
            s = 1 << it
            usable = fp & np.isfinite(c).all(-1) & np.isfinite(v)
            Y = luminance(c)
            lum = usable if guided else np.zeros((h, w), bool)
            gl = np.zeros((h, w), f32)
            if guided:
                pv, pw = np.zeros((h, w), f32), np.zeros((h, w), f32)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        m = shifted(usable, dx, dy, False)
                        wt = G3[dy + 1] * G3[dx + 1]
                        pv = np.where(m, pv + wt * shifted(v, dx, dy, 0), pv)
                        pw = np.where(m, pw + wt, pw)
                vv = np.where(pw > 0, pv / pw, v)
                gl = kl / (vv + f32(1e-6))
            sw, sv = np.zeros((h, w), f32), np.zeros((h, w), f32)
            acc = np.zeros((h, w, 3), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = s * dx, s * dy
                    m = shifted(usable, ox, oy, False)
                    if not m.any():
                        continue
                    cq, vq = shifted(c, ox, oy, 0), shifted(v, ox, oy, 0)
                    Nq, Aq, Zq = shifted(N, ox, oy, 0), shifted(A, ox, oy, 0), shifted(Z, ox, oy, 0)
                    d = N - Nq
                    dn = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    d = A - Aq
                    da = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    d = Z - Zq
                    dz = d * d
                    t = ((one + dn * kn) * (one + da * ka)) * (one + dz * kz)
                    if guided:
                        dl = Y - luminance(cq)
                        t = np.where(lum, t * (one + (dl * dl) * gl), t)
                    t = t * t
                    t = t * t
                    wt = (H5[dy + 2] * H5[dx + 2]) / t
                    ok = m & (wt > 0)
                    sw = np.where(ok, sw + wt, sw)
                    acc = np.where(ok[..., None], acc + wt[..., None] * cq, acc)
                    sv = np.where(ok, sv + (wt * wt) * vq, sv)
            has = fp & (sw > 0)
            c = np.where(has[..., None], acc / sw[..., None], c).astype(f32)
            v = np.where(has, sv / (sw * sw), v).astype(f32)
    out = image.copy()
    out[..., :3] = c
    return out


def rel_mse(x, ref):
    x, ref = np.asarray(x[..., :3], np.float64), np.asarray(ref[..., :3], np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))
