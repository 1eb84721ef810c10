"""Device-resident input pipeline: train from a dataset directory (the reference's ``--dataset_dir``).

The reference loads every sample from disk at every step (model.py:219-256, utils.py:167-233): ``imread``, two anti-aliased
skimage ``resize`` calls, a coin-flip ``fliplr``.  Here each PNG is decoded ONCE (PIL) and kept on the device as uint8;
a batch is then produced by ``sgg_resample_u8`` (csrc/resample.hip) straight into the buffers the step reads, in the
networks' internal layout, so nothing is decoded, converted or copied on the host per step.

``skimage.transform.resize`` (0.16.2 defaults: order=1, mode='reflect', anti_aliasing=True) is restated from its
documentation and source [3P-recall] -- skimage is not a dependency: per axis with scale s = n_in / n_out >= 1, a Gaussian of
sigma = (s - 1) / 2 truncated at 4 sigma with scipy's 'mirror' boundary, then linear interpolation at
x_src = (x_dst + 0.5) * s - 0.5.  Both are linear and separable, so a chain of resizes is ONE banded matrix per axis
(``band_table``), built in float64 and stored as f32 weights + int32 starts.
"""
from __future__ import annotations

import functools
import glob
import os

import numpy as np


# ------------------------------------------------------------------------------------------------ band tables (host, NumPy)
def _mirror(i, n):
    """scipy.ndimage mode='mirror': reflect about the centre of the edge samples (d c b | a b c d | c b a)."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def _gauss_matrix(n, sigma):
    """(n, n) float64 matrix of scipy.ndimage.gaussian_filter1d(sigma, truncate=4.0, mode='mirror')."""
    if sigma <= 0:
        return np.eye(n)
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x * x)
    w /= w.sum()
    G = np.zeros((n, n))
    rows = np.arange(n)
    for d, wd in zip(range(-radius, radius + 1), w):
        np.add.at(G, (rows, _mirror(rows + d, n)), wd)
    return G


def _linear_matrix(n_in, n_out):
    """(n_out, n_in) float64 matrix of linear interpolation at x_src = (x_dst + 0.5) * s - 0.5, s = n_in / n_out >= 1."""
    s = n_in / n_out
    x = (np.arange(n_out, dtype=np.float64) + 0.5) * s - 0.5
    x0 = np.floor(x).astype(np.int64)
    f = x - x0
    L = np.zeros((n_out, n_in))
    rows = np.arange(n_out)
    np.add.at(L, (rows, np.clip(x0, 0, n_in - 1)), 1.0 - f)
    np.add.at(L, (rows, np.clip(x0 + 1, 0, n_in - 1)), f)
    return L


def resize_matrix(n_in, n_out):
    """One axis of one skimage ``resize`` call as a dense (n_out, n_in) float64 matrix.  Upscaling is refused."""
    if n_out > n_in:
        raise ValueError(f"resize {n_in} -> {n_out}: upscaling (scale < 1) is out of scope")
    if n_out <= 0:
        raise ValueError("empty axis")
    return _linear_matrix(n_in, n_out) @ _gauss_matrix(n_in, (n_in / n_out - 1.0) / 2.0)


def axis_matrix(sizes):
    """A chain of resizes n0 -> n1 -> ... (float64 intermediates, no rounding in between) as one dense matrix."""
    sizes = [int(v) for v in sizes]
    A = np.eye(sizes[0])
    for a, b in zip(sizes[:-1], sizes[1:]):
        A = resize_matrix(a, b) @ A
    return A


@functools.lru_cache(maxsize=64)
def band_table64(sizes):
    """axis_matrix(sizes) as a band in float64: (weights (n_out, taps), starts int32 (n_out,), step) with
    out[i] = sum_k weights[i, k] * in[starts[i] + k], starts[i] + taps <= n_in, step = max(starts[i + 1] - starts[i]).
    Depends on the sizes only: cached per source shape."""
    A = axis_matrix(sizes)
    n_out, n_in = A.shape
    nz = A != 0.0
    first = nz.argmax(axis=1)
    last = n_in - 1 - nz[:, ::-1].argmax(axis=1)
    taps = int((last - first).max()) + 1
    starts = np.minimum(first, n_in - taps).astype(np.int32)
    w = np.ascontiguousarray(np.take_along_axis(A, starts[:, None].astype(np.int64) + np.arange(taps)[None, :], axis=1))
    assert np.count_nonzero(w) == np.count_nonzero(A)            # the band holds every non-zero of the matrix
    step = int(np.diff(starts).max()) if n_out > 1 else 0
    w.setflags(write=False)
    starts.setflags(write=False)
    return w, starts, max(step, 0)


@functools.lru_cache(maxsize=64)
def band_table(sizes):
    """band_table64 as the kernel takes it: f32 weights, int32 starts, step."""
    w, starts, step = band_table64(tuple(sizes))
    w32 = w.astype(np.float32)
    w32.setflags(write=False)
    return w32, starts, step


def train_tables(H0, W0, H, W):
    """(rows, cols) band tables of load_train_data's chain: resize(x, (H0, H0)) -- rows unchanged -- then resize(x, (H, W))."""
    return band_table((H0, H0, H)), band_table((W0, H0, W))


def test_tables(H0, W0, H, W):
    """load_test_data's single resize (H0, W0) -> (H, W)."""
    return band_table((H0, H)), band_table((W0, W))


def apply_tables(x, rows, cols):
    """NumPy reference application of two band tables to (H0, W0, C) uint8 / float data -> float64 (H, W, C) in [0, 1] for
    uint8 input (the /255 of the reference's img_as_float).  Host-side statement of what sgg_resample_u8 computes."""
    x = np.asarray(x)
    v = x.astype(np.float64) / 255.0 if x.dtype == np.uint8 else x.astype(np.float64)
    (rw, rs, _), (cw, cs, _) = rows, cols
    h = np.zeros((v.shape[0], cw.shape[0]) + v.shape[2:])
    for k in range(cw.shape[1]):
        h += cw[:, k].astype(np.float64).reshape((1, -1) + (1,) * (v.ndim - 2)) * v[:, cs + k]
    out = np.zeros((rw.shape[0],) + h.shape[1:])
    for k in range(rw.shape[1]):
        out += rw[:, k].astype(np.float64).reshape((-1,) + (1,) * (v.ndim - 1)) * h[rs + k]
    return out


# ------------------------------------------------------------------------------------------------ augmented copy (host, NumPy)
# The reference trains on every file twice: as loaded, and through DataAugmentation.augmentation_func (utils.py:80-103,
# 180-182): iaa.Sequential([Fliplr(0.5), Crop(percent=(0.2, 0.4)), Affine(translate_percent +-0.1, rotate +-1 deg)],
# random_order=True) on the squared image A = resize(src, (H0, H0)), S = H0.  imgaug is not a dependency and its RNG cannot
# be reproduced, so the rule is restated (deviation D6).  Coordinates are continuous, pixel centres at +0.5;
# every operation is its OUTPUT -> INPUT map g:
#   op 0  Fliplr : coin set: (x, y) -> (S - x, y)
#   op 1  Crop   : fractions top, right, bottom, left in [0.2, 0.4) -> whole pixels t, r, b, l = rint(f * S) (size is kept):
#                  (x, y) -> (l + x * (S - l - r) / S, t + y * (S - t - b) / S)
#   op 2  Affine : forward = rotate by `angle` about (S/2, S/2) (x' = c x - s y, y' = s x + c y), then translate by
#                  (tx * S, ty * S); g is its inverse.  cval = 0: where g's result lies outside [0, S] x [0, S] the pixel is 0
#                  on every channel (tested in the affine's own input frame).
# `perm` lists the operations in the order they are applied to the image, so an output pixel p samples A at
# g_perm[0](g_perm[1](g_perm[2](p))) -- with ONE bilinear interpolation (edge clamp) where imgaug interpolates per operation.
AUG_FLIP, AUG_CROP, AUG_AFFINE = 0, 1, 2
AUG_CROP_RANGE, AUG_TRANSLATE_RANGE, AUG_ROTATE_RANGE = (0.2, 0.4), (-0.1, 0.1), (-1.0, 1.0)


def draw_augment_params(rng, n):
    """The draws of n augmented copies from ``rng`` (a np.random.RandomState), per copy in this order: the permutation of the
    three operations, the flip coin (random_sample() < 0.5), the crop fractions top, right, bottom, left, the translation
    tx, ty, the angle in degrees, and the loader's own flip (random_sample() > 0.5, utils.py:201) -- 11 scalar draws after
    the permutation.  -> dict of arrays with leading dimension n."""
    p = {"perm": np.zeros((n, 3), np.int64), "flip": np.zeros(n, bool), "crop": np.zeros((n, 4)), "translate": np.zeros((n, 2)),
         "angle": np.zeros(n), "loader_flip": np.zeros(n, bool)}
    for i in range(n):
        p["perm"][i] = rng.permutation(3)
        p["flip"][i] = rng.random_sample() < 0.5
        p["crop"][i] = [rng.uniform(*AUG_CROP_RANGE) for _ in range(4)]
        p["translate"][i] = [rng.uniform(*AUG_TRANSLATE_RANGE) for _ in range(2)]
        p["angle"][i] = rng.uniform(*AUG_ROTATE_RANGE)
        p["loader_flip"][i] = rng.random_sample() > 0.5
    return p


def identity_augment_params(n):
    """Parameters under which every operation is the identity map (tests, and the documentation of the dict's layout)."""
    return {"perm": np.tile(np.arange(3), (n, 1)), "flip": np.zeros(n, bool), "crop": np.zeros((n, 4)),
            "translate": np.zeros((n, 2)), "angle": np.zeros(n), "loader_flip": np.zeros(n, bool)}


def _op_matrix(op, S, flip, crop, translate, angle):
    """One operation's output -> input map as a 3x3 homogeneous float64 matrix."""
    S = float(S)
    if op == AUG_FLIP:
        return np.array([[-1.0, 0.0, S], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) if flip else np.eye(3)
    if op == AUG_CROP:
        t, r, b, l = (float(np.rint(f * S)) for f in crop)
        return np.array([[(S - l - r) / S, 0.0, l], [0.0, (S - t - b) / S, t], [0.0, 0.0, 1.0]])
    c, s = np.cos(np.deg2rad(angle)), np.sin(np.deg2rad(angle))
    Rinv = np.array([[c, s], [-s, c]])                       # inverse of x' = c x - s y, y' = s x + c y
    ctr = np.array([S / 2.0, S / 2.0])
    M = np.eye(3)
    M[:2, :2] = Rinv
    M[:2, 2] = ctr - Rinv @ (np.array([translate[0] * S, translate[1] * S]) + ctr)
    return M


def augment_matrices(params, S):
    """-> (n, 2, 2, 3) float64.  [:, 0] maps an output point to the affine operation's input frame (the zero-fill test),
    [:, 1] maps it to the squared image A (the sample point).  Both are products of the per-operation maps in drawn order."""
    n = len(params["angle"])
    out = np.zeros((n, 2, 2, 3))
    for i in range(n):
        perm = [int(v) for v in params["perm"][i]]
        g = [_op_matrix(op, S, params["flip"][i], params["crop"][i], params["translate"][i], params["angle"][i]) for op in perm]
        k = perm.index(AUG_AFFINE)
        fill = np.eye(3)
        for m in g[k:]:
            fill = fill @ m
        full = np.eye(3)
        for m in g:
            full = full @ m
        out[i, 0], out[i, 1] = fill[:2], full[:2]
    return out


def _augment_points(matrices, S):
    """(inside (S, S) bool, sx, sy): the zero-fill decision and the sample point of every output pixel centre, each
    coordinate as (m0 * px + m1 * py) + m2 in that order -- the arithmetic sgg_warp_affine_u8 repeats."""
    assert np.shape(matrices) == (2, 2, 3)
    py, px = np.meshgrid(np.arange(S) + 0.5, np.arange(S) + 0.5, indexing="ij")
    (fx, fy), (sx, sy) = [[(m[r, 0] * px + m[r, 1] * py) + m[r, 2] for r in range(2)] for m in np.asarray(matrices, np.float64)]
    return (fx >= 0.0) & (fx <= S) & (fy >= 0.0) & (fy <= S), sx, sy


def augment_inside(matrices, S):
    """(S, S) bool: False where the affine operation's zero fill applies, decided exactly as the kernel decides it."""
    return _augment_points(matrices, S)[0]


def apply_augment(A, matrices):
    """The warp of ONE sample, float64: A (S, S, C) float, matrices (2, 2, 3) from augment_matrices -> (S, S, C).  Every
    coordinate is (m0 * px + m1 * py) + m2 in that order with (px, py) = (x + 0.5, y + 0.5), which is what the kernel
    evaluates (sgg_warp_affine_u8), so both make the same zero-fill and floor decisions."""
    A = np.asarray(A, dtype=np.float64)
    S = A.shape[0]
    assert A.shape[1] == S
    inside, sx_, sy_ = _augment_points(matrices, S)
    u, v = sx_ - 0.5, sy_ - 0.5
    x0, y0 = np.floor(u), np.floor(v)
    wx, wy = u - x0, v - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(x0, 0, S - 1), np.clip(x0 + 1, 0, S - 1)
    ya, yb = np.clip(y0, 0, S - 1), np.clip(y0 + 1, 0, S - 1)
    e = (Ellipsis, None)
    out = (((1.0 - wy) * (1.0 - wx))[e] * A[ya, xa] + ((1.0 - wy) * wx)[e] * A[ya, xb]
           + (wy * (1.0 - wx))[e] * A[yb, xa] + (wy * wx)[e] * A[yb, xb])
    return np.where(inside[e], out, 0.0)


def interleave(plain, copies):
    """Per-sample values of the plain samples and of their copies -> row order of the doubled batch [s0, aug(s0), s1, ...]."""
    return np.stack([np.asarray(plain), np.asarray(copies)], axis=1).reshape(-1)


def warp_window(matrices, tile=(16, 64)):
    """(rows, cols) of A that one tile of tile = (rows, cols) output pixels can touch under any of the (n, 2, 2, 3) matrices:
    the maps are affine, so the extent is the same for every tile; + 4: the second bilinear neighbour, the two floors, one pixel of slack."""
    m = np.abs(np.asarray(matrices, np.float64).reshape(-1, 2, 2, 3)[:, 1])
    th, tw = tile
    cols = int(np.ceil((m[:, 0, 0] * (tw - 1) + m[:, 0, 1] * (th - 1)).max())) + 4
    rows = int(np.ceil((m[:, 1, 0] * (tw - 1) + m[:, 1, 1] * (th - 1)).max())) + 4
    return rows, cols


def warp_window_bound(S, tile=(16, 64)):
    """warp_window's largest value over the parameter ranges, so that the warp's launch (LDS size included) is the same at
    every step of every epoch: the linear part of the composed map is a flip, a crop scale and a rotation in some order, every
    entry at most scale * cos / scale * sin in size, with scale <= 1 - 2 * rint(0.2 S) / S <= 0.6 + 1 / S and |angle| <= 1 deg."""
    th, tw = tile
    scale = 1.0 - 2.0 * np.rint(AUG_CROP_RANGE[0] * S) / S
    c, s = np.cos(np.deg2rad(AUG_ROTATE_RANGE[1])), np.sin(np.deg2rad(AUG_ROTATE_RANGE[1]))
    return int(np.ceil(scale * (c * (th - 1) + s * (tw - 1)))) + 4, int(np.ceil(scale * (c * (tw - 1) + s * (th - 1)))) + 4


# ------------------------------------------------------------------------------------------------ files
def sibling(path, split, suffix):
    """The reference's rule (utils.py:169-170, 121, 146): ``image_path.replace("trainA", "trainA_seg")`` on the whole path."""
    return path.replace(split, split + suffix)


def list_files(root, split):
    return sorted(glob.glob(os.path.join(root, split, "*.*")))


def decode(path, kind):
    """PNG -> uint8 array as the reference's imread hands it to resize: image RGB, colour label RGB or RGBA (a palette
    label becomes RGB), class map one channel."""
    from PIL import Image
    with Image.open(path) as im:
        if kind == "class":
            return np.asarray(im if im.mode == "L" else im.convert("L"), dtype=np.uint8)
        if im.mode not in ("RGB", "RGBA"):
            im = im.convert("RGB")
        return np.asarray(im, dtype=np.uint8)


class DatasetCache:
    """Every sample of ``<root>/<split>`` (+ ``<split>_seg``, ``<split>_seg_class``) decoded once and held on the device as
    uint8, grouped by source shape: ``image[i] / label[i] / classmap[i]`` = (stack tensor, index inside the stack).
    Memory: 3 + 4 (RGBA label) + 1 bytes per source pixel (100 Cityscapes files of 2048x1024: 1.7 GB)."""

    def __init__(self, root, split="trainA", device="cuda", max_files=None, with_class=True):
        import torch
        self.root, self.split, self.device = root, split, torch.device(device)
        files = list_files(root, split)
        if max_files is not None:
            files = files[:int(max_files)]
        if not files:
            raise FileNotFoundError(f"no files under {os.path.join(root, split)}")
        self.files = files
        self.seg_files = [sibling(f, split, "_seg") for f in files]
        self.class_files = [sibling(f, split, "_seg_class") for f in files] if with_class else None
        self.stacks = {}
        self.image = self._load(self.files, "image")
        self.label = self._load(self.seg_files, "label")
        self.classmap = self._load(self.class_files, "class") if with_class else None

    @classmethod
    def from_arrays(cls, images, labels, classmaps, device="cuda", names=None):
        """A cache of already decoded uint8 arrays (synthetic data, benchmarks): images (H0,W0,3), labels (H0,W0,3|4),
        classmaps (H0,W0)."""
        import torch
        self = cls.__new__(cls)
        self.root, self.split, self.device = None, None, torch.device(device)
        self.files = list(names) if names is not None else ["sample_%05d.png" % i for i in range(len(images))]
        self.seg_files = self.class_files = None
        self.stacks = {}
        self.image = self._group(images, "image")
        self.label = self._group(labels, "label")
        self.classmap = self._group(classmaps, "class") if classmaps is not None else None
        return self

    def __len__(self):
        return len(self.files)

    def _load(self, paths, role):
        return self._group((decode(p, "class" if role == "class" else "image") for p in paths), role)

    def _group(self, arrays, role):
        """-> per file (stack key, index in stack); self.stacks[(role, H0, W0[, Cs])] = uint8 device tensor (M, H0, W0[, Cs])."""
        import torch
        groups, where = {}, []
        for a in arrays:
            a = np.ascontiguousarray(a, dtype=np.uint8)
            key = (role,) + a.shape
            g = groups.setdefault(key, [])
            where.append((key, len(g)))
            g.append(a)
        for key, arrs in groups.items():
            self.stacks[key] = torch.as_tensor(np.stack(arrs)).to(self.device)
        return where

    def shapes(self):
        return sorted({k[1:] for k in self.stacks})


def _device_tables(tables, device):
    import torch
    return tuple((torch.as_tensor(np.array(w)).to(device), torch.as_tensor(np.array(s)).to(device), step) for w, s, step in tables)


def mask_grid(model, H, W):
    """Spatial size of the semantic mask: the discriminator's output map, or (H/34, W/34) where that is 1x1 (utils.py:197)."""
    mh, mw = model.discriminator.out_hw(H, W)
    if (mh, mw) == (1, 1):
        mh, mw = round(H / 34), round(W / 34)
    return mh, mw


class _Domain:
    """One domain's cache + the persistent batch buffers it fills."""

    def __init__(self, model, args, cache, tag, augment=False):
        import torch
        from . import kernels as K
        from .segment_class import one_hot_mask
        self.cache, self.tag, self.augment = cache, tag, bool(augment)
        H, W = args.image_height, args.image_width
        N = args.batch_size * (2 if self.augment else 1)          # augmented: [s0, aug(s0), s1, aug(s1), ...] (model.py:236-244)
        dev = cache.device
        self.C = args.input_nc
        if self.augment and self.C > 3:
            raise ValueError("augment: the warp carries three channels (the reference's RGB image and colour label)")
        self.tables, self.aug_tables = {}, {}
        for key in {k for k, _ in cache.image} | {k for k, _ in cache.label}:
            H0, W0 = key[1], key[2]
            if (H0, W0) not in self.tables:
                self.tables[(H0, W0)] = _device_tables(train_tables(H0, W0, H, W), dev)
                if self.augment:      # the chain cut at the squared image: columns W0 -> H0 (warp), then (H0, H0) -> (H, W)
                    self.aug_tables[(H0, W0)] = _device_tables((band_table((W0, H0)), band_table((H0, H)), band_table((H0, W))), dev)
            if key[3] < self.C:
                raise ValueError(f"{cache.root}: {key[3]}-channel sources cannot fill input_nc={self.C}")
        self.real = torch.zeros((N, H, W, K.cpad(self.C)), dtype=model.dtype, device=dev)
        # augmented: the plain samples are resampled densely (the same launches as without augmentation) and copied to the even rows
        self._plain_tmp = torch.empty((args.batch_size, H, W, K.cpad(self.C)), dtype=model.dtype, device=dev) if self.augment else None
        self.seg = torch.zeros_like(self.real)
        mh, mw = mask_grid(model, H, W)
        nc = args.segment_class
        self.mask = torch.zeros((N, mh, mw, nc), dtype=torch.float32, device=dev)
        # per-file masks, once: sgg_onehot_resample of each class map (a few KB per file); a step gathers and flips them
        self.mask_table = torch.empty((len(cache), mh, mw, nc), dtype=torch.float32, device=dev)
        by_group = {}
        for f, (key, i) in enumerate(cache.classmap):
            by_group.setdefault(key, []).append((f, i))
        for key, pairs in by_group.items():
            m = one_hot_mask(cache.stacks[key], mh, mw, nc)
            fi = torch.as_tensor([f for f, _ in pairs], device=dev)
            gi = torch.as_tensor([i for _, i in pairs], device=dev)
            self.mask_table[fi] = m[gi]
        self._mask_tmp = torch.empty_like(self.mask)

    def buffers(self):
        return {"real_" + self.tag: self.real, "seg_" + self.tag: self.seg, "mask_" + self.tag: self.mask}

    def plan(self, order, aug=None):
        """Host part of an epoch: per-sample stack indices of the chosen files, uploaded once per epoch.  ``aug``: the
        parameters of the samples' augmented copies (draw_augment_params) -> their matrices per source, the LDS window of the
        warp (its bound over the parameter ranges, not the drawn values), and every file twice for the doubled batch's masks."""
        import torch
        c = self.cache
        dev = c.device
        img = np.array([c.image[f][1] for f in order], dtype=np.int32)
        lab = np.array([c.label[f][1] for f in order], dtype=np.int32)
        p = {"order": list(order), "img": torch.as_tensor(img).to(dev), "lab": torch.as_tensor(lab).to(dev),
             "file": torch.as_tensor(np.asarray(order, dtype=np.int32)).to(dev)}
        if aug is not None:
            one = lambda i: {k: v[i:i + 1] for k, v in aug.items()}
            for role, where in (("img", c.image), ("lab", c.label)):       # the squared side S = H0 of each sample's own source
                m = np.concatenate([augment_matrices(one(i), where[f][0][1]) for i, f in enumerate(order)]) if len(order) else np.zeros((0, 2, 2, 3))
                p[role + "_mats"] = torch.as_tensor(m).to(dev)
                win = (1, 1)
                for S in {where[f][0][1] for f in order}:                  # constant per source height, whatever was drawn
                    win = tuple(max(a, b) for a, b in zip(win, warp_window_bound(S)))
                assert not len(order) or all(a <= b for a, b in zip(warp_window(m), win))
                p[role + "_win"] = win
            p["file2"] = torch.as_tensor(np.repeat(np.asarray(order, dtype=np.int32), 2)).to(dev)
        return p

    def _resample(self, where, plan_idx, order, lo, hi, flips, out):
        """Runs of consecutive samples that share a source stack -> one launch each (one launch when shapes are uniform)."""
        from . import kernels as K
        a = lo
        while a < hi:
            key = where[order[a]][0]
            b = a + 1
            while b < hi and where[order[b]][0] == key:
                b += 1
            rows, cols = self.tables[(key[1], key[2])]
            K.resample_u8(self.cache.stacks[key], plan_idx[a:b], flips[a:b], rows, cols, out[a - lo:b - lo], self.C)
            a = b

    def fill(self, plan, lo, hi, flips, flips_bool):
        import torch
        c = self.cache
        self._resample(c.image, plan["img"], plan["order"], lo, hi, flips, self.real)
        self._resample(c.label, plan["lab"], plan["order"], lo, hi, flips, self.seg)
        torch.index_select(self.mask_table, 0, plan["file"][lo:hi], out=self._mask_tmp)
        torch.where(flips_bool[lo:hi].view(-1, 1, 1, 1), self._mask_tmp.flip(2), self._mask_tmp, out=self.mask)


    def fill_augmented(self, plan, lo, hi, flips, aug_flips, flips2_bool, inter):
        """The doubled batch: plain sample i -> row 2i (fill's own launches into a dense temporary, then one strided copy: the
        same bits), its copy -> row 2i + 1 through warp + resample_f32; masks are the per-file masks, not warped (the
        reference augments image and label only), each with its own row's flip."""
        import torch
        from . import kernels as K
        c, order, n = self.cache, plan["order"], hi - lo
        for where, role, out in ((c.image, "img", self.real), (c.label, "lab", self.seg)):
            idx, mats, win = plan[role], plan[role + "_mats"], plan[role + "_win"]
            self._resample(where, idx, order, lo, hi, flips, self._plain_tmp)
            out[0::2].copy_(self._plain_tmp)
            a = lo
            while a < hi:
                key = where[order[a]][0]
                b = a + 1
                while b < hi and where[order[b]][0] == key:
                    b += 1
                square, arows, acols = self.aug_tables[(key[1], key[2])]
                tmp = inter(key[1], n)[:b - a]
                K.warp_affine_u8(c.stacks[key], idx[a:b], mats[a:b], square, win, tmp)
                K.resample_f32(tmp, aug_flips[a:b], arows, acols, out[2 * (a - lo) + 1::2][:b - a], self.C)
                a = b
        torch.index_select(self.mask_table, 0, plan["file2"][2 * lo:2 * hi], out=self._mask_tmp)
        torch.where(flips2_bool[2 * lo:2 * hi].view(-1, 1, 1, 1), self._mask_tmp.flip(2), self._mask_tmp, out=self.mask)


class _Epoch:
    """One epoch's batches: sized, and lazily filled -- every yielded dict holds the SAME device tensors, refilled in place
    just before the yield, so a consumer must finish (enqueue) a step before asking for the next batch."""

    def __init__(self, owner, plans, flips, n_batches):
        self._o, self._plans, self._flips, self._n = owner, plans, flips, n_batches

    def __len__(self):
        return self._n

    def __iter__(self):
        for b in range(self._n):
            yield self._o._fill(self._plans, self._flips, b)


class DirectoryBatches:
    """``batches(epoch)`` for ``sggan.train`` from one (reference mode) or two (cycle mode) ``DatasetCache``s.

    Protocol of model.py:219-228 + utils.py:201: per epoch the sorted file list is shuffled with ``rng.shuffle`` (domain A,
    then domain B), ``min(len, train_size) // batch_size`` batches are cut from its head, and every sample takes one
    ``rng.random_sample() > 0.5`` flip draw in batch order (cycle mode: one draw per A/B pair, applied to both, as upstream
    SG-GAN's paired loader does).  ``rng`` is a ``np.random.RandomState`` (default seed 19; the reference leaves NumPy unseeded).
    With ``model.use_graph`` the buffers become the recorded step's static inputs, so a replayed step reads them directly.

    ``augment=True`` (the reference's default --use_augmentation branch, model.py:234-244): every sample is followed by its
    augmented copy, so the buffers hold ``2 * batch_size`` samples ``[s0, aug(s0), s1, aug(s1), ...]`` and the number of steps
    is unchanged.  Everything about the copies is drawn from a SECOND stream ``aug_rng`` (default seed 23) after the epoch's
    ``rng`` draws -- draw_augment_params for domain A's copies, then for domain B's -- so ``rng`` and with it the plain samples
    are what they are without augmentation.  A copy's loader flip is its own draw (cycle mode: domain A's draw serves the A/B
    pair, domain B's is drawn and unused)."""

    def __init__(self, model, args, cache_A, cache_B=None, rng=None, augment=False, aug_rng=None):
        import torch
        self.model, self.args = model, args
        self.rng = rng if rng is not None else np.random.RandomState(19)
        self.augment = bool(augment)
        self.aug_rng = aug_rng if aug_rng is not None else np.random.RandomState(23)
        self.cycle = bool(getattr(args, "cycle", False))
        if self.cycle and cache_B is None:
            raise ValueError("cycle mode needs a second domain (cache_B)")
        self.domains = [_Domain(model, args, cache_A, "A", self.augment)] + \
                       ([_Domain(model, args, cache_B, "B", self.augment)] if self.cycle else [])
        self._inter = {}                      # the warp's f32 intermediates (batch_size, S, S, 4), one per source height
        self.batch = {}
        for d in self.domains:
            self.batch.update(d.buffers())
        self.device = cache_A.device
        self._torch = torch
        if getattr(model, "use_graph", False):
            model.adopt_inputs(**self.batch)

    def intermediate(self, S, n):
        """The warp's output buffer for n samples of side S: allocated once, shared by images, labels and both domains (one
        stream: a launch is done with it before the next one writes it)."""
        t = self._inter.get(S)
        if t is None or t.shape[0] < n:
            t = self._inter[S] = self._torch.empty((n, S, S, 4), dtype=self._torch.float32, device=self.device)
        return t

    def epoch_plan(self):
        """The host-side draws of one epoch from ``rng``: ([file order per domain], flips (n_batches * batch_size,) bool,
        n_batches) -- the same with and without augmentation."""
        a = self.args
        orders = []
        for d in self.domains:
            order = list(range(len(d.cache)))
            self.rng.shuffle(order)
            orders.append(order)
        n_batches = min(min(len(o) for o in orders), a.train_size) // a.batch_size
        flips = np.array([self.rng.random_sample() > 0.5 for _ in range(n_batches * a.batch_size)], dtype=bool)
        return [o[:n_batches * a.batch_size] for o in orders], flips, n_batches

    def augment_plan(self, orders):
        """The copies' draws of one epoch from ``aug_rng``, made after epoch_plan's: [draw_augment_params dict per domain],
        domain A's first, one set of parameters per sample of ``orders``."""
        return [draw_augment_params(self.aug_rng, len(o)) for o in orders]

    def __call__(self, epoch):
        torch = self._torch
        if self.augment:
            orders, flips, n = self.epoch_plan()
            aug = self.augment_plan(orders)
            plans = [d.plan(o, g) for d, o, g in zip(self.domains, orders, aug)]
            aug_flips = aug[0]["loader_flip"]                              # one loader flip per A/B pair
            both = interleave(flips, aug_flips)
            up = lambda x: torch.as_tensor(x.astype(np.int32)).to(self.device)
            return _Epoch(self, plans, (up(flips), up(aug_flips), up(both) != 0), n)
        orders, flips, n = self.epoch_plan()
        plans = [d.plan(o) for d, o in zip(self.domains, orders)]
        f32 = torch.as_tensor(flips.astype(np.int32)).to(self.device)
        return _Epoch(self, plans, (f32, f32 != 0), n)

    def _fill(self, plans, flips, b):
        N = self.args.batch_size
        for d, p in zip(self.domains, plans):
            if self.augment:
                d.fill_augmented(p, b * N, (b + 1) * N, flips[0], flips[1], flips[2], self.intermediate)
            else:
                d.fill(p, b * N, (b + 1) * N, flips[0], flips[1])
        return self.batch


def directory_test_samples(args, cache):
    """``samples(epoch)`` for ``test_during_train`` / ``test``: (name, image (H,W,3), colour label (H,W,3)) float32 in [0,1]
    through load_test_data's one-stage resize (utils.py:116-122).  The reference's ``resize(x, [H, W, 3])`` also interpolates
    an RGBA label across its channel axis; here the first three channels are resized on their own (deviation D8).
    A cache built with ``with_class=True`` adds a fourth element: load_test_data's full-resolution one-hot class mask
    (utils.py:146-150) as float32 (H,W,segment_class), through segment_class.one_hot_mask (deviation D1) -- what
    ``test_during_train`` needs for its CRF scores (--crf)."""
    import torch
    from . import kernels as K
    from .segment_class import one_hot_mask

    def gen(epoch=0):
        H, W = args.image_height, args.image_width
        dev = cache.device
        one = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.empty((1, H, W, K.cpad(3)), dtype=torch.float32, device=dev)
        for f, name in enumerate(cache.files):
            pair = []
            for where in (cache.image, cache.label):
                key, i = where[f]
                rows, cols = _device_tables(test_tables(key[1], key[2], H, W), dev)
                K.resample_u8(cache.stacks[key], torch.full_like(one, i), one, rows, cols, out, 3)
                pair.append(K.unpad_channels(out, 3)[0].cpu().numpy())
            if cache.classmap is None:
                yield os.path.basename(name), pair[0], pair[1]
            else:
                key, i = cache.classmap[f]
                mask = one_hot_mask(cache.stacks[key][i:i + 1], H, W, args.segment_class)
                yield os.path.basename(name), pair[0], pair[1], mask[0].cpu().numpy()
    return gen


def directory_images(args, root, split, count, device):
    """``images()`` yielding the first ``count`` files of ``<root>/<split>`` in sorted order as (H,W,3) float32 in [0,1] at the test
    size, through the resize of ``directory_test_samples`` -- the unpaired reals of the test pass's SWD.  The
    files are decoded once and held on the device as uint8."""
    import torch
    from . import kernels as K
    dev = torch.device(device)
    files = list_files(root, split)[:int(count)]
    if not files:
        raise FileNotFoundError(f"no files under {os.path.join(root, split)}")
    stacks = [torch.as_tensor(np.array(decode(f, "image"))[None]).to(dev) for f in files]       # (a copy: a decoded PNG is read-only)

    def gen():
        H, W = args.image_height, args.image_width
        zero = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.empty((1, H, W, K.cpad(3)), dtype=torch.float32, device=dev)
        for st in stacks:
            rows, cols = _device_tables(test_tables(st.shape[1], st.shape[2], H, W), dev)
            K.resample_u8(st, zero, zero, rows, cols, out, 3)
            yield K.unpad_channels(out, 3)[0].cpu().numpy()
    return gen


def resolve_root(dataset_dir, split="trainA"):
    """The reference reads ``./datasets/<dataset_dir>/<split>`` (model.py:220); a path that holds ``<split>`` itself wins.
    None: neither exists (the caller keeps its synthetic sources)."""
    for root in (dataset_dir, os.path.join(".", "datasets", dataset_dir)):
        if os.path.isdir(os.path.join(root, split)):
            return root
    return None
