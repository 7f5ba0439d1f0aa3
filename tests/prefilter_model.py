"""numpy restatement of the single-precision pre-filter that K1 (k_hist, k_hist_planes) and k_inquad run before the reference's
doubles (the constants: csrc/ssd_prexy.h; the device code: csrc/ssd_prefilter.h, pre_range and pre_pixel), shared by tests/test_prexy.py and
tests/test_gpu_prefilter_regimes.py.

Each FMA is an exact float64 product-and-sum rounded once to float32: the product of two float32 values is exact in float64 and
the sum's own float64 rounding is 2^-29 of a float32 ulp, far inside the bounds' slack.  `kernel_decisions` follows the kernel's
lane masks one by one; its `drop` argument removes one band at a time, so that a test can count the points a kernel without that
band would get wrong."""
import numpy as np


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def chain(c_row, p):
    """the kernel's three FMAs of one x / y row (pre_xy) on float32 inputs p [n, 3]; c_row = (c0, c1, c2, c3) float32"""
    f = np.float64
    r = (f(c_row[2]) * p[:, 2].astype(f) + f(c_row[3])).astype(np.float32)
    r = (f(c_row[1]) * p[:, 1].astype(f) + r.astype(f)).astype(np.float32)
    return (f(c_row[0]) * p[:, 0].astype(f) + r.astype(f)).astype(np.float32)


def fma32(a, x, c):
    """fl32(a * x + c) on float32 operands"""
    return (np.float64(a) * np.asarray(x).astype(np.float64) + np.asarray(c, dtype=np.float32).astype(np.float64)).astype(np.float32)


def t_chain(zc, p):
    """the z row: the height above zMin in bins"""
    return fma32(zc[0], p[:, 0], fma32(zc[1], p[:, 1], fma32(zc[2], p[:, 2], np.full(len(p), zc[3], np.float32))))


def threshold(neg_k, M3, h0):
    """h = fma(M3, negK, h0): half a bin (pixel) minus the bound for the point's magnitude"""
    return fma32(neg_k, M3, np.full(len(M3), h0, np.float32))


def sure(t, M3, neg_k, h0):
    """the kernel's certainty test: |fract(t) - 1/2| < h0 + neg_k * M3, all in float32; False for NaNs"""
    with np.errstate(invalid="ignore", over="ignore"):
        g = ((t - np.floor(t)).astype(np.float32) - np.float32(0.5)).astype(np.float32)
        return np.abs(g) < threshold(neg_k, M3, h0)


def absmax3(p):
    """v_max3_f32 on |x|, |y|, |z|: a NaN operand is ignored"""
    return np.fmax(np.fmax(np.abs(p[:, 0]), np.abs(p[:, 1])), np.abs(p[:, 2])).astype(np.float32)


def reference(lim, a, b, recip, p):
    """pointcloud.cpp:143-178 / transformation.h:59-64 in the reference's doubles, operation by operation:
    lim = (x_min, x_max, y_min, y_max, z_min, z_max) -> (in range, height bin (0 where out of range))"""
    x_min, x_max, y_min, y_max, z_min, z_max = lim
    x, y, z = (p[:, i].astype(np.float64) for i in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        wx = ((a[0, 0] * x + a[0, 1] * y) + a[0, 2] * z) + b[0]
        wy = ((a[1, 0] * x + a[1, 1] * y) + a[1, 2] * z) + b[1]
        wz = ((a[2, 0] * x + a[2, 1] * y) + a[2, 2] * z) + b[2]
        ok = (p[:, 2] > 0) & (wx > x_min) & (wx < x_max) & (wy > y_min) & (wy < y_max) & (wz > z_min) & (wz < z_max)
        hb = np.where(ok, (wz - z_min) * recip, 0.0).astype(np.int64)
    return ok, hb


def kernel_decisions(Q, Z, lim, a, b, recip, p, drop=()):
    """the in-range decision and the height bin K1 / k_inquad reach for camera floats p [n, 3] with the constants Q (prexy_host) and
    Z (prez_host), as their lane masks do: single precision where it is sure, the reference's doubles for the rest.
    drop removes a band (the per-point test that sends points to the doubles):
      "top"  the band at the top of a z range that is not a whole number of bins (zCheckTop, SSD_SABOTAGE_PRE & 8),
      "far"  the magnitude test of the input (checkInput: mFar, SSD_SABOTAGE_PRE & 16),
      "xy"   the whole x / y band and the magnitude test: lo = hi = 1/2 on the same d,
      "z"    the whole z band: a point is sure unless t is an integer, with the z row rounded from a and b where make_pre_z zeroed it.
    -> (in range, bin (0 where out of range), the points that took the doubles)"""
    with np.errstate(invalid="ignore", over="ignore"):
        valid = p[:, 2] > 0
        c = Q["c"]
        dx, dy = chain(c[:, 0], p), chain(c[:, 1], p)
        M = np.maximum(np.abs(dx), np.abs(dy))
        lo, hi = (np.float32(0.5), np.float32(0.5)) if "xy" in drop else (Q["lo"], Q["hi"])
        inxy = M < lo
        maybexy = ~(M > hi)
        M3 = absmax3(p)
        checks = Q["check_input"] or Z["z_check_top"]
        if checks and Q["check_input"] and "far" not in drop and "xy" not in drop:
            far = ~(M3 <= Q["max_input"])
            inxy &= ~far
            maybexy |= far
        zc, neg_k, h0, z_top, check_top = Z["zc"], Z["z_neg_k"], Z["z_h0"], Z["z_top"], Z["z_check_top"]
        if "z" in drop:
            neg_k, h0 = np.float32(0.0), np.float32(0.5)
            if not np.any(zc):
                z_min, z_max = lim[4], lim[5]
                zc = np.array([a[2, 0] * recip, a[2, 1] * recip, a[2, 2] * recip, (b[2] - z_min) * recip], dtype=np.float32)
                top = (z_max - z_min) * recip
                check_top, z_top = top != np.rint(top), np.float32(top if top != np.rint(top) else np.rint(top))
        t = t_chain(zc, p)
        h = threshold(neg_k, M3, h0)
        g = ((t - np.floor(t)).astype(np.float32) - np.float32(0.5)).astype(np.float32)
        surez = np.abs(g) < h
        inz = (t >= 0) & ~np.signbit(t) & (t < z_top)
        if checks and check_top and "top" not in drop:
            surez &= np.abs((t - z_top).astype(np.float32)) > (np.float32(0.5) - h).astype(np.float32)
        bsp = np.where(t >= 0, np.floor(np.nan_to_num(t, nan=0.0, posinf=0.0)), 0.0).astype(np.int64)
        in_sure = valid & inz & inxy & surez
        slow = valid & maybexy & (~surez | (inz & ~inxy))
    ok, hb = reference(lim, a, b, recip, p)
    inr = in_sure | (slow & ok)
    hbin = np.where(slow, hb, np.where(inr, bsp, 0))
    return inr, hbin, slow


def histogram(inr, hbin, n_bins):
    return np.bincount(hbin[inr], minlength=n_bins)[:n_bins] if inr.any() else np.zeros(n_bins, dtype=np.int64)
