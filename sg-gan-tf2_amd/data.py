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

    def __init__(self, model, args, cache, tag):
        import torch
        from . import kernels as K
        from .segment_class import one_hot_mask
        self.cache, self.tag = cache, tag
        N, H, W = args.batch_size, args.image_height, args.image_width
        dev = cache.device
        self.C = args.input_nc
        self.tables = {}
        for key in {k for k, _ in cache.image} | {k for k, _ in cache.label}:
            H0, W0 = key[1], key[2]
            if (H0, W0) not in self.tables:
                self.tables[(H0, W0)] = _device_tables(train_tables(H0, W0, H, W), dev)
            if key[3] < self.C:
                raise ValueError(f"{cache.root}: {key[3]}-channel sources cannot fill input_nc={self.C}")
        self.real = torch.zeros((N, H, W, K.cpad(self.C)), dtype=model.dtype, device=dev)
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

    def plan(self, order):
        """Host part of an epoch: per-sample stack indices of the chosen files, uploaded once per epoch."""
        import torch
        c = self.cache
        dev = c.device
        img = np.array([c.image[f][1] for f in order], dtype=np.int32)
        lab = np.array([c.label[f][1] for f in order], dtype=np.int32)
        return {"order": list(order), "img": torch.as_tensor(img).to(dev), "lab": torch.as_tensor(lab).to(dev),
                "file": torch.as_tensor(np.asarray(order, dtype=np.int32)).to(dev)}

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
    With ``model.use_graph`` the buffers become the recorded step's static inputs, so a replayed step reads them directly."""

    def __init__(self, model, args, cache_A, cache_B=None, rng=None):
        import torch
        self.model, self.args = model, args
        self.rng = rng if rng is not None else np.random.RandomState(19)
        self.cycle = bool(getattr(args, "cycle", False))
        if self.cycle and cache_B is None:
            raise ValueError("cycle mode needs a second domain (cache_B)")
        self.domains = [_Domain(model, args, cache_A, "A")] + ([_Domain(model, args, cache_B, "B")] if self.cycle else [])
        self.batch = {}
        for d in self.domains:
            self.batch.update(d.buffers())
        self.device = cache_A.device
        self._torch = torch
        if getattr(model, "use_graph", False):
            model.adopt_inputs(**self.batch)

    def epoch_plan(self):
        """The host-side draws of one epoch: ([file order per domain], flips (n_batches * batch_size,) bool, n_batches)."""
        a = self.args
        orders = []
        for d in self.domains:
            order = list(range(len(d.cache)))
            self.rng.shuffle(order)
            orders.append(order)
        n_batches = min(min(len(o) for o in orders), a.train_size) // a.batch_size
        flips = np.array([self.rng.random_sample() > 0.5 for _ in range(n_batches * a.batch_size)], dtype=bool)
        return [o[:n_batches * a.batch_size] for o in orders], flips, n_batches

    def __call__(self, epoch):
        torch = self._torch
        orders, flips, n = self.epoch_plan()
        plans = [d.plan(o) for d, o in zip(self.domains, orders)]
        f32 = torch.as_tensor(flips.astype(np.int32)).to(self.device)
        return _Epoch(self, plans, (f32, f32 != 0), n)

    def _fill(self, plans, flips, b):
        N = self.args.batch_size
        for d, p in zip(self.domains, plans):
            d.fill(p, b * N, (b + 1) * N, flips[0], flips[1])
        return self.batch


def directory_test_samples(args, cache):
    """``samples(epoch)`` for ``test_during_train`` / ``test``: (name, image (H,W,3), colour label (H,W,3)) float32 in [0,1]
    through load_test_data's one-stage resize (utils.py:116-122).  The reference's ``resize(x, [H, W, 3])`` also interpolates
    an RGBA label across its channel axis; here the first three channels are resized on their own (deviation D8)."""
    import torch
    from . import kernels as K

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
            yield os.path.basename(name), pair[0], pair[1]
    return gen


def resolve_root(dataset_dir, split="trainA"):
    """The reference reads ``./datasets/<dataset_dir>/<split>`` (model.py:220); a path that holds ``<split>`` itself wins.
    None: neither exists (the caller keeps its synthetic sources)."""
    for root in (dataset_dir, os.path.join(".", "datasets", dataset_dir)):
        if os.path.isdir(os.path.join(root, split)):
            return root
    return None
