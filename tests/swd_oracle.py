"""NumPy statement of the test pass's sliced Wasserstein distance (csrc/swd.hip), test infrastructure only.

The semantics are those of PGGAN's ``metrics/sliced_wasserstein.py`` (Karras et al. 2018, section 5), restated from memory; every
recalled point is tagged [3P-recall].  Each stage is stated twice and the two statements are pinned to each other by
tests/test_swd_cpu.py: the pyramid with separable filters and as the direct 5x5 sum in reversed tap order (bit-equal: with
integer inputs every intermediate is an exact dyadic rational), the descriptor gather by fancy indexing and by loops.  The patch
positions come from tests/diffaug_oracle.py's Philox.  ``dtype`` selects float64 (the oracle) or ``np.longdouble`` (the
yardstick eps64 is measured against).
"""
import json
import os

import numpy as np

from tests.diffaug_oracle import philox4x32_10

F32, F64, LD = np.float32, np.float64, np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swd_eps.json")
TAPS = (1, 4, 6, 4, 1)              # / 16: the binomial filter of the Laplacian pyramid [3P-recall]
K = 147                             # 7 x 7 x 3 [3P-recall: 7x7 neighbourhoods, 128 per image and level, 4 x 128 directions]


# ------------------------------------------------------------------------------------------------ quantisation
def quantise(x):
    """The 8-bit colours of a float image in [-1,1]: (int)(((x + 1) * 0.5) * 255) in float32, clamped to 0..255, NaN -> 0
    (utils.inverse_transform as sgg_image_quality documents it); uint8 passes through."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x
    v = ((x.astype(F32) + F32(1)) * F32(0.5)) * F32(255)
    out = np.zeros(v.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        hi, mid = v >= F32(255), (v > F32(0)) & (v < F32(255))
    out[hi] = 255
    out[mid] = v[mid].astype(np.int32).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ pyramid
def mirror(i, n):
    """Mirror border without edge repeat: -1 -> 1, n -> n - 2 [3P-recall: scipy / OpenCV 'reflect101', PGGAN's mode='mirror']."""
    i = np.asarray(i)
    return np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def _filter_axis(x, axis, taps):
    n = x.shape[axis]
    out = np.zeros_like(x)
    for a, t in enumerate(taps):
        out = out + t * np.take(x, mirror(np.arange(n) + a - 2, n), axis=axis)
    return out


def filter_separable(x, scale):
    """t (x) t over the last two axes, rows first: scale * sum."""
    return _filter_axis(_filter_axis(x, -1, TAPS), -2, TAPS) * scale


def filter_direct(x, scale):
    """The same as one 5x5 sum, taps in REVERSED order."""
    h, w = x.shape[-2:]
    out = np.zeros_like(x)
    for a in range(4, -1, -1):
        for b in range(4, -1, -1):
            ys, xs = mirror(np.arange(h) + a - 2, h), mirror(np.arange(w) + b - 2, w)
            out = out + (TAPS[a] * TAPS[b]) * x[..., ys[:, None], xs[None, :]]
    return out * scale


def down(x, direct=False):
    """G_k = the filtered G_{k-1}, every second row and column from 0 [3P-recall: pyr_down]."""
    f = (filter_direct if direct else filter_separable)(x, x.dtype.type(1) / 256)
    return f[..., ::2, ::2]


def up(x, direct=False):
    """Zero-stuff to twice the size (Z[2i,2j] = x[i,j]) and filter Z with 4 (t (x) t) under the mirror rule on Z [3P-recall: pyr_up]."""
    z = np.zeros(x.shape[:-2] + (2 * x.shape[-2], 2 * x.shape[-1]), x.dtype)
    z[..., ::2, ::2] = x
    return (filter_direct if direct else filter_separable)(z, x.dtype.type(4) / 256)


def pyramid(img_u8, levels, direct=False, dtype=F64):
    """img (N,H,W,3|4) uint8 -> [Lap_0 ... Lap_{levels-1}], each (N,3,h,w) in ``dtype``: Lap_k = G_k - up(G_{k+1}), the last one
    G_{levels-1} [3P-recall: laplacian_pyramid]."""
    g = [np.ascontiguousarray(np.asarray(img_u8)[..., :3].transpose(0, 3, 1, 2)).astype(dtype)]
    for _ in range(levels - 1):
        g.append(down(g[-1], direct))
    return [g[k] - up(g[k + 1], direct) for k in range(levels - 1)] + [g[-1]]


def pyramid_flat(img, levels):
    """What sgg_swd_pyramid writes: (N, E) float32, the levels concatenated, each planar."""
    lv = pyramid(quantise(img), levels)
    return np.concatenate([l.reshape(l.shape[0], -1) for l in lv], axis=1).astype(F32)


def default_levels(H, W):
    best = 0
    for L in range(1, 6):
        if H % (1 << (L - 1)) == 0 and W % (1 << (L - 1)) == 0 and (min(H, W) >> (L - 1)) >= 16:
            best = L
    return best


# ------------------------------------------------------------------------------------------------ descriptors
def mulhi32(a, b):
    return (int(a) * int(b)) >> 32


def positions(seed, g, level, patches, h, w):
    """(patches, 2) patch centres (cy, cx) of image g at a level of h x w: key (seed, 1), counter (g, level, p // 2, 0); words 0, 1
    place patch 2 (p // 2), words 2, 3 patch 2 (p // 2) + 1."""
    out = np.empty((patches, 2), np.int64)
    for p in range(patches):
        r = philox4x32_10((g & 0xFFFFFFFF, level, p // 2, 0), (seed, 1))
        wy, wx = (r[2], r[3]) if p & 1 else (r[0], r[1])
        out[p] = 3 + mulhi32(wy, h - 6), 3 + mulhi32(wx, w - 6)
    return out


def descriptors(level_planar, level, patches, seed, image_offset=0):
    """level_planar (N,3,h,w) -> (N * patches, 147), rows [i * patches + p], flattened (channel, y, x) [3P-recall]; fancy indexing."""
    N, _, h, w = level_planar.shape
    d = np.arange(-3, 4)
    rows = []
    for i in range(N):
        pos = positions(seed, image_offset + i, level, patches, h, w)
        ys, xs = pos[:, 0, None] + d[None], pos[:, 1, None] + d[None]                    # (P,7)
        patch = level_planar[i][:, ys[:, :, None], xs[:, None, :]]                       # (3,P,7,7)
        rows.append(patch.transpose(1, 0, 2, 3).reshape(patches, K))
    return np.concatenate(rows)


def descriptors_loops(level_planar, level, patches, seed, image_offset=0):
    N, _, h, w = level_planar.shape
    out = np.empty((N * patches, K), level_planar.dtype)
    for i in range(N):
        pos = positions(seed, image_offset + i, level, patches, h, w)
        for p in range(patches):
            cy, cx = pos[p]
            for c in range(3):
                for y in range(7):
                    for x in range(7):
                        out[i * patches + p, (c * 7 + y) * 7 + x] = level_planar[i, c, cy - 3 + y, cx - 3 + x]
    return out


# ------------------------------------------------------------------------------------------------ normalise, project, sort, distance
def moments(desc, dtype=F64):
    """(3,2): per colour channel (mean, population standard deviation) over all M * 49 values [3P-recall: ddof 0]."""
    d = np.asarray(desc).astype(dtype).reshape(len(desc), 3, 49)
    mean = d.mean(axis=(0, 2))
    std = np.sqrt(((d - mean[None, :, None]) ** 2).mean(axis=(0, 2)))
    return np.stack([mean, std], axis=1)


def normalise(desc, dtype=F64):
    """(desc - mean_c) / std_c; a channel with deviation 0 gives zeros (PGGAN would divide by zero)."""
    m = moments(desc, dtype)
    d = np.asarray(desc).astype(dtype).reshape(len(desc), 3, 49) - m[None, :, 0, None]
    safe = np.where(m[:, 1] == 0, dtype(1), m[:, 1])
    z = np.where((m[:, 1] == 0)[None, :, None], dtype(0), d / safe[None, :, None])
    return z.reshape(len(desc), K)


def project(z, dirs):
    """(D, M): proj[d][m] = sum_k z[m][k] dirs[k][d], k ascending, in z's type (no BLAS: the order is the statement's own).
    Also returns sum_k |z_k dirs_k|, the scale a projection's rounding error is measured against."""
    dirs = np.asarray(dirs).astype(z.dtype)
    acc, mag = np.zeros((dirs.shape[1], z.shape[0]), z.dtype), np.zeros((dirs.shape[1], z.shape[0]), z.dtype)
    for k in range(K):
        term = dirs[k][:, None] * z[None, :, k]
        acc, mag = acc + term, mag + np.abs(term)
    return acc, mag


def distance(pa, pb):
    """1e3 * sum_d sum_m |sort(a) - sort(b)| / (D M) [3P-recall: the mean over repeats of means; every repeat has the same count]."""
    D, M = pa.shape
    return pa.dtype.type(1e3) * np.abs(np.sort(pa, axis=1) - np.sort(pb, axis=1)).sum() / (D * M)


def score(desc_a, desc_b, dirs, dtype=F64):
    return distance(project(normalise(desc_a, dtype), dirs)[0], project(normalise(desc_b, dtype), dirs)[0])


def directions(D, seed=19):
    """metric.swd_directions restated: Gaussian columns from a seeded torch generator, unit length in double, stored as float32."""
    import torch
    g = torch.randn((K, int(D)), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64)
    return (g / g.norm(dim=0, keepdim=True)).to(torch.float32).numpy()


def swd(fakes, reals, levels, patches, dirs, seed=19, dtype=F64):
    """The whole score of two image sets (N,H,W,C): ([per-level values], mean)."""
    n = min(len(fakes), len(reals))
    pf, pr = pyramid(quantise(fakes[:n]), levels), pyramid(quantise(reals[:n]), levels)
    vals = []
    for l in range(levels):
        da = descriptors(pf[l], l, patches, seed).astype(F32)         # the pyramid is stored as float32
        db = descriptors(pr[l], l, patches, seed).astype(F32)
        vals.append(score(da, db, dirs, dtype))
    return vals, sum(vals) / len(vals)


# ------------------------------------------------------------------------------------------------ shared inputs and eps64
SCORE_CASES = [(M, D) for M in (3, 33, 768) for D in (1, 128, 512)]


def case_descriptors(M, D):
    """Two descriptor sets (M,147) float32 for the projection / score case (M, D): values of the size a pyramid level holds --
    a small spread on a large mean in channel 0 (a coarsest level), zero-mean detail in the others."""
    rng = np.random.default_rng(1000 * M + D)
    def one(shift):
        d = rng.normal(0.0, 20.0, (M, 3, 49))
        d[:, 0] = 127.0 + shift + rng.normal(0.0, 4.0, (M, 49))
        d[:, 2] *= 1.0 + shift
        return d.reshape(M, K).astype(F32)
    return one(0.0), one(0.25)


def image_case():
    """The full-pipeline case: two sets of three 32x48 images, two levels, 11 patches (M = 33), 128 directions."""
    rng = np.random.default_rng(77)
    smooth = np.linspace(0, 200, 48)[None, None, :, None] + np.linspace(0, 40, 32)[None, :, None, None]
    fakes = np.clip(smooth + rng.integers(0, 16, (3, 32, 48, 3)), 0, 255).astype(np.uint8)
    reals = rng.integers(0, 256, (3, 32, 48, 3)).astype(np.uint8)
    return dict(fakes=fakes, reals=reals, levels=2, patches=11, repeats=1, dirs_per_repeat=128, seed=19)


def measured_eps64():
    """{"proj", "score"}: the worst difference between the float64 statement and the same statement in np.longdouble over the
    shared inputs -- projections relative to sum_k |z_k d_k|, scores relative to the score."""
    eps_p = eps_s = 0.0
    for M, D in SCORE_CASES:
        a, b = case_descriptors(M, D)
        dirs = directions(D)
        got = []
        for dt in (F64, LD):
            pa, mag = project(normalise(a, dt), dirs)
            pb, mag_b = project(normalise(b, dt), dirs)
            got.append((pa, pb, mag, mag_b, distance(pa, pb)))
        (pa, pb, _, _, s64), (qa, qb, mag, mag_b, sld) = got
        eps_p = max(eps_p, float((np.abs(pa - qa) / mag).max()), float((np.abs(pb - qb) / mag_b).max()))
        eps_s = max(eps_s, float(abs(s64 - sld) / sld))
    c = image_case()
    dirs = directions(c["repeats"] * c["dirs_per_repeat"], c["seed"])
    v64, m64 = swd(c["fakes"], c["reals"], c["levels"], c["patches"], dirs, c["seed"], F64)
    vld, mld = swd(c["fakes"], c["reals"], c["levels"], c["patches"], dirs, c["seed"], LD)
    for x, y in list(zip(v64, vld)) + [(m64, mld)]:
        eps_s = max(eps_s, float(abs(x - y) / y))
    return {"proj": eps_p, "score": eps_s}


def golden_eps64():
    with open(GOLDEN) as f:
        return json.load(f)
