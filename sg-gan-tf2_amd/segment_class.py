"""Colour -> class-index masks on the GPU -- mirror of the reference's ``segment_class.py``.

``cityscape()`` / ``A_maskmap()`` return the same 21-entry (R,G,B) -> class dictionary
(segment_class.py:60-73; read back from the kernel's own table so the two cannot drift);
``preprocess(img)`` is the per-pixel lookup of segment_class.py:87-97 as one HIP kernel
(bit exact, default class 0, alpha ignored).  PNG I/O and the process pool
(segment_class.py:79-99) are host tooling and out of scope.
"""
from __future__ import annotations

import ctypes as C
from collections import defaultdict

import numpy as np
import torch

from . import _abi as A
from . import kernels as K

num_seg_masks = 8       # segment_class.py:10


def cityscape():
    """segment_class.py:60-70."""
    keys = (C.c_uint32 * 32)()
    vals = (C.c_uint8 * 32)()
    n = A.lib().sgg_seg_class_table(keys, vals, 32)
    if n <= 0:
        raise A.SggError("sgg_seg_class_table failed")
    m = defaultdict(int)
    for i in range(n):
        k = int(keys[i])
        m[((k >> 16) & 255, (k >> 8) & 255, k & 255)] = int(vals[i])
    return m


def A_maskmap():
    """segment_class.py:72-73."""
    return cityscape()


def preprocess(img, device="cuda"):
    """segment_class.py:87-97: uint8 (M,N,3|4) [or a batch (B,M,N,3|4)] -> uint8 class indices, on the GPU.
    Accepts numpy or torch; returns a torch uint8 tensor on `device`."""
    t = img if isinstance(img, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(img))
    if t.dtype != torch.uint8 or t.shape[-1] < 3:
        raise ValueError("expected uint8 image(s) with >= 3 channels")
    return K.seg_class_map(t.to(device).contiguous())


def one_hot_mask(seg_class, out_h, out_w, num_classes=num_seg_masks):
    """utils.py:158-165 (one_hot) + utils.py:197-199 (zoom to the mask grid), fused: uint8 (B,M,N) class
    indices -> float32 (B,out_h,out_w,num_classes) one-hot of the align-corners nearest resample
    (deviation D1)."""
    t = seg_class if isinstance(seg_class, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(seg_class))
    if t.dim() == 2:
        t = t[None]
    return K.onehot_resample(t.to(torch.uint8).cuda().contiguous(), int(out_h), int(out_w), int(num_classes))


def palette():
    """The library's built-in colour table as ``(keys uint32[21], classes uint8[21])``, key = R<<16 | G<<8 | B -- the palette
    ``metric.palette_labels`` uses when none is given (read from the library: there is one copy of the table)."""
    keys = (C.c_uint32 * 64)()
    vals = (C.c_uint8 * 64)()
    n = A.lib().sgg_seg_class_table(keys, vals, 64)
    if n <= 0:
        raise A.SggError("sgg_seg_class_table failed")
    return np.array(keys[:n], dtype=np.uint32), np.array(vals[:n], dtype=np.uint8)


def _pairs_of(cache_or_pairs):
    """(colour label (H,W,3|4) uint8, class map (H,W) uint8) tensors of a data.DatasetCache or of an iterable of array pairs."""
    if hasattr(cache_or_pairs, "stacks"):
        cache = cache_or_pairs
        if cache.classmap is None:
            raise ValueError("learn_palette: the cache holds no class maps (build it with with_class=True)")
        for (lkey, li), (ckey, ci) in zip(cache.label, cache.classmap):
            yield cache.stacks[lkey][li], cache.stacks[ckey][ci]
    else:
        for label, classmap in cache_or_pairs:
            as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(np.array(a))
            yield as_t(label), as_t(classmap)


def learn_palette(cache_or_pairs, max_entries=64):
    """The palette of a dataset, learned from its own source-resolution (colour label, class map) pairs: every
    distinct label colour maps to the class most of its pixels carry (ties to the lowest class); entries are ordered by
    descending pixel count, then ascending key, and cut at ``max_entries``.  Alpha is ignored.  Returns
    ``(keys uint32[K], classes uint8[K])``.  Runs once per dataset: one torch.unique per pair where the tensors live (the
    device for a DatasetCache), merged on the host."""
    votes = defaultdict(lambda: defaultdict(int))                      # key -> class -> pixels
    for label, classmap in _pairs_of(cache_or_pairs):
        if label.dtype != torch.uint8 or label.dim() != 3 or label.shape[-1] < 3 or tuple(classmap.shape) != tuple(label.shape[:2]):
            raise ValueError(f"learn_palette: label {tuple(label.shape)} / class map {tuple(classmap.shape)} do not pair")
        rgb = label[..., :3].to(torch.int64)
        code = (((rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]) << 8) | classmap.to(torch.int64)
        pairs, counts = torch.unique(code.reshape(-1), return_counts=True)
        for pc, n in zip(pairs.cpu().tolist(), counts.cpu().tolist()):
            votes[pc >> 8][pc & 255] += n
    entries = []
    for key, per_class in votes.items():
        top = max(per_class.values())
        entries.append((-sum(per_class.values()), key, min(c for c, n in per_class.items() if n == top)))
    entries.sort()
    entries = entries[:int(max_entries)]
    return np.array([e[1] for e in entries], dtype=np.uint32), np.array([e[2] for e in entries], dtype=np.uint8)
