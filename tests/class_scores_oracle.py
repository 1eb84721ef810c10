"""NumPy restatement of the class-level evaluation rules (csrc/evalseg.hip) -- integer throughout, the
probabilities in float64.  Test infrastructure only.

    colour   float input: q_c = (int)(((x_c + 1.f) * 0.5f) * 255.f) in float32, clamped to 0..255, NaN -> 0; uint8 input: the byte
    d2_k     = sum_c (q_c - key_k.c)^2, key = R<<16 | G<<8 | B
    winner   = the smallest d2, ties to the lowest k
    label    = class[winner] if max_dist2 < 0 or d2 <= max_dist2 else other_class
"""
import os
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "city_small")
NONE = np.iinfo(np.int64).max


def quantise(x):
    """float image (..., C>=3) -> int64 (..., 3) 8-bit colours."""
    x = np.asarray(x, dtype=np.float32)[..., :3]
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((x + np.float32(1.0)) * np.float32(0.5)) * np.float32(255.0)
    assert v.dtype == np.float32
    q = np.zeros(v.shape, dtype=np.int64)
    ok = ~np.isnan(v)
    q[ok] = np.clip(np.trunc(v[ok].astype(np.float64)), 0, 255).astype(np.int64)       # (int) truncates toward zero, then the clamp
    return q


def colours(img):
    """(..., C) float or uint8 image -> int64 (..., 3)."""
    img = np.asarray(img)
    return img[..., :3].astype(np.int64) if img.dtype == np.uint8 else quantise(img)


def key_rgb(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], axis=-1)


def distances(q, keys):
    """int64 (..., K) squared distances of the colours q (..., 3) to every palette key."""
    d = q[..., None, :] - key_rgb(keys)
    return (d * d).sum(axis=-1)


def labels(img, keys, classes, other_class=0, max_dist2=-1):
    d = distances(colours(img), keys)
    k = np.argmin(d, axis=-1)                                  # the first minimum: ties to the lowest k
    best = np.take_along_axis(d, k[..., None], axis=-1)[..., 0]
    lab = np.asarray(classes, dtype=np.int64)[k]
    if max_dist2 >= 0:
        lab = np.where(best <= max_dist2, lab, other_class)
    return lab.astype(np.int32)


def hist(truth, pred, n_class, select=None):
    """int64 (n_class, n_class): hist[t, p] += 1 over the pixels with t, p < n_class (and select != 0)."""
    t, p = np.asarray(truth, dtype=np.int64).ravel(), np.asarray(pred, dtype=np.int64).ravel()
    ok = (t < n_class) & (p < n_class) & (t >= 0) & (p >= 0)
    if select is not None:
        ok &= np.asarray(select).ravel() != 0
    return np.bincount(n_class * t[ok] + p[ok], minlength=n_class * n_class).reshape(n_class, n_class)


def band(cls, r):
    """uint8 (N,H,W): 1 iff some in-image pixel with |dy|, |dx| <= r has a class other than the centre's."""
    cls = np.asarray(cls)
    N, H, W = cls.shape
    out = np.zeros((N, H, W), dtype=np.uint8)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))          # centres whose neighbour is inside
            yn, xn = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
            if ys.start >= ys.stop or xs.start >= xs.stop:
                continue
            out[:, ys, xs] |= (cls[:, ys, xs] != cls[:, yn, xn]).astype(np.uint8)
    return out


def class_distances(img, keys, classes, n_class, other_class=0, max_dist2=-1):
    """int64 (..., n_class): the smallest d2 over the entries of each class; NONE where a class has no distance.  other_class
    without an entry takes the pseudo-distance max_dist2 where that is >= 0."""
    d = distances(colours(img), keys)
    classes = np.asarray(classes, dtype=np.int64)
    m = np.full(d.shape[:-1] + (n_class,), NONE, dtype=np.int64)
    for c in range(n_class):
        mine = classes == c
        if mine.any():
            m[..., c] = d[..., mine].min(axis=-1)
        elif c == other_class and max_dist2 >= 0:
            m[..., c] = max_dist2
    return m


def probs(img, keys, classes, n_class, sigma=32.0, other_class=0, max_dist2=-1):
    """float64 (N, n_class, H, W) of an image (N,H,W,C): e_c = exp(-(m_c - m_min) / (2 sigma^2)), 0 without a distance, p = e / sum."""
    m = class_distances(img, keys, classes, n_class, other_class, max_dist2)
    have = m != NONE
    mmin = np.where(have, m, NONE).min(axis=-1, keepdims=True)
    e = np.where(have, np.exp(-np.where(have, m - mmin, 0).astype(np.float64) / (2.0 * float(sigma) ** 2)), 0.0)
    p = e / e.sum(axis=-1, keepdims=True)
    return np.moveaxis(p, -1, 1)


def learn_palette(pairs, max_entries=64):
    """(keys uint32[K], classes uint8[K]) from (colour label (H,W,3|4) uint8, class map (H,W)) pairs: each distinct colour maps
    to its majority class (ties to the lowest class); descending pixel count, then ascending key; cut at max_entries."""
    votes = defaultdict(lambda: defaultdict(int))
    for label, classmap in pairs:
        label, classmap = np.asarray(label), np.asarray(classmap)
        rgb = label[..., :3].astype(np.int64)
        key = (rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]
        code, count = np.unique((key << 8) | classmap.astype(np.int64), return_counts=True)
        for kc, n in zip(code.tolist(), count.tolist()):
            votes[kc >> 8][kc & 255] += n
    entries = []
    for k, per_class in votes.items():
        best = max(per_class.values())
        entries.append((-sum(per_class.values()), k, min(c for c, n in per_class.items() if n == best)))
    entries.sort()
    entries = entries[:max_entries]
    return np.array([e[1] for e in entries], dtype=np.uint32), np.array([e[2] for e in entries], dtype=np.uint8)


def city_pairs():
    """The three (colour label, class map) pairs of tests/golden/city_small, as decoded uint8 arrays."""
    from PIL import Image
    out = []
    for split in ("trainA", "testA"):
        for name in sorted(os.listdir(os.path.join(FIX, split + "_seg"))):
            label = Image.open(os.path.join(FIX, split + "_seg", name))
            if label.mode not in ("RGB", "RGBA"):
                label = label.convert("RGB")
            out.append((np.asarray(label, dtype=np.uint8), np.asarray(Image.open(os.path.join(FIX, split + "_seg_class", name)), dtype=np.uint8)))
    return out


_CITY = {}


def city_palette():
    """learn_palette of the fixture pairs, computed once."""
    if "p" not in _CITY:
        _CITY["p"] = learn_palette(city_pairs())
    return _CITY["p"]


def random_palette(K, n_class, seed):
    """K entries over n_class classes with two built-in ties: entries 0 / 1 are two colours 4 apart on one axis with different
    classes (their midpoint is equidistant), and -- from K = 4 -- entries 2 / 3 hold the SAME colour with different classes."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (K, 3))
    cls = rng.integers(0, n_class, K)
    if K >= 2:
        rgb[0] = (100, 50, 200); rgb[1] = (104, 50, 200)
        cls[0], cls[1] = (n_class - 1, 0) if n_class > 1 else (0, 0)
    if K >= 4:
        rgb[3] = rgb[2]
        cls[2], cls[3] = (min(1, n_class - 1), 0)
    keys = (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]
    return keys.astype(np.uint32), cls.astype(np.uint8)
