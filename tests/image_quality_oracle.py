"""Float64 NumPy statement of the paired image-quality scores (csrc/imgqual.hip), written from the definition:
every 11 x 11 window that lies inside the image is weighted densely by the outer product of the Gaussian window -- not
separably, so it shares no summation order with the kernel.

    q      = the 8-bit colour: the byte of a uint8 image; (int)(((x + 1) * 0.5) * 255) in float32, clamped to 0..255, NaN -> 0
    sad    = sum |qa - qb|,  ssd = sum (qa - qb)^2                   over all H * W * 3 values (integers)
    S      = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))   per window and channel,
             ux = E[x], vx = E[xx] - ux^2, vxy = E[xy] - ux uy under w (x) w,  w_k ~ exp(-k^2 / (2 * 1.5^2)), k = -5..5, sum 1
             (the variances are taken in their CENTRED form E[(x - ux)^2], E[(x - ux)(y - uy)] -- the same quantities, since w sums
             to 1, without the cancellation of E[xx] - ux^2: the reference is then good to ~1e-15 where the kernel's one-pass
             form carries ~1e-12, and two constant images give the closed form (2 c1 c2 + C1) / (c1^2 + c2^2 + C1) to 1e-15)
    MAE = sad / (3HW),  MSE = ssd / (3HW),  PSNR = 10 log10(255^2 / MSE),  SSIM = sum S / (3 (H-10) (W-10))
"""
import numpy as np

R, TAPS, SIGMA = 5, 11, 1.5
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def window():
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return w / w.sum()


def quantise(x):
    """int64 8-bit colours of the first three channels of ``x`` (N,H,W,C) or (H,W,C): uint8 as it is, float by the f32 rule."""
    x = np.asarray(x)
    x = x[None] if x.ndim == 3 else x
    x = x[..., :3]
    if x.dtype == np.uint8:
        return x.astype(np.int64)
    v = ((x.astype(np.float32) + np.float32(1.0)) * np.float32(0.5)) * np.float32(255.0)
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore"):                                   # NaN fails both comparisons -> 0
        q = np.where(v >= np.float32(255.0), 255.0, np.where(v > np.float32(0.0), np.trunc(v), 0.0))
    return q.astype(np.int64)


def ssim_map(qa, qb):
    """S (N, H-10, W-10, 3) float64 of two int (N,H,W,3) arrays: dense windows over the valid region."""
    x, y = qa.astype(np.float64), qb.astype(np.float64)
    N, H, W, _ = x.shape
    vh, vw = H - 2 * R, W - 2 * R
    assert vh >= 1 and vw >= 1
    w2 = np.outer(window(), window())
    shifted = lambda s, dy, dx: s[:, dy:dy + vh, dx:dx + vw, :]
    ux, uy = np.zeros((N, vh, vw, 3)), np.zeros((N, vh, vw, 3))
    for dy in range(TAPS):
        for dx in range(TAPS):
            ux += w2[dy, dx] * shifted(x, dy, dx)
            uy += w2[dy, dx] * shifted(y, dy, dx)
    vx, vy, vxy = np.zeros_like(ux), np.zeros_like(ux), np.zeros_like(ux)
    for dy in range(TAPS):
        for dx in range(TAPS):
            cx, cy = shifted(x, dy, dx) - ux, shifted(y, dy, dx) - uy
            vx += w2[dy, dx] * (cx * cx)
            vy += w2[dy, dx] * (cy * cy)
            vxy += w2[dy, dx] * (cx * cy)
    return ((2.0 * (ux * uy) + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def sums(a, b):
    """float64 (N,3): {sad, ssd, sum of the SSIM map} -- what sgg_image_quality writes."""
    qa, qb = quantise(a), quantise(b)
    assert qa.shape == qb.shape
    d = qa - qb
    N = qa.shape[0]
    out = np.empty((N, 3), dtype=np.float64)
    out[:, 0] = np.abs(d).reshape(N, -1).sum(axis=1)
    out[:, 1] = (d * d).reshape(N, -1).sum(axis=1)
    out[:, 2] = ssim_map(qa, qb).reshape(N, -1).sum(axis=1)
    return out


def counts(H, W):
    """(values of the integer sums, values of the SSIM sum) per image."""
    return 3 * H * W, 3 * (H - 2 * R) * (W - 2 * R)


def scores(a, b):
    """Per-image arrays {"MAE", "MSE", "PSNR", "SSIM"}."""
    qa = quantise(a)
    s = sums(a, b)
    n_all, n_valid = counts(qa.shape[1], qa.shape[2])
    mse = s[:, 1] / n_all
    with np.errstate(divide="ignore"):
        psnr = np.where(mse > 0, 10.0 * np.log10(255.0 ** 2 / np.where(mse > 0, mse, 1.0)), np.inf)
    return {"MAE": s[:, 0] / n_all, "MSE": mse, "PSNR": psnr, "SSIM": s[:, 2] / n_valid}


def pooled(rows, H, W):
    """The test pass's three scalars from per-image sums ``rows`` (M,3) of equal-sized images: MAE and PSNR pooled over all
    values (PSNR of a zero MSE: the finite bound 10 log10(255^2 * count)), SSIM the mean of the per-image SSIMs."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    n_all, n_valid = counts(H, W)
    total = n_all * len(rows)
    mse = rows[:, 1].sum() / total
    psnr = 10.0 * np.log10(255.0 ** 2 / mse) if mse > 0 else 10.0 * np.log10(255.0 ** 2 * total)
    return {"MAE": rows[:, 0].sum() / total, "PSNR": psnr, "SSIM": float(np.mean(rows[:, 2] / n_valid))}
