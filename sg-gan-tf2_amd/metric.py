"""Evaluation metrics -- mirror of the NumPy part of the reference's ``metric.py`` (next-row SURVEY.md 8(f)4).

``_fast_hist`` / ``scores`` (metric.py:18-47) with the confusion matrix accumulated on the GPU (integer atomics:
exact and order-independent) and ``scores_seg_fake`` (metric.py:71-77).

``dense_crf`` (metric.py:49-69) runs on the GPU as an EXACT mean-field fully connected CRF (csrc/crf.hip): the same unary,
Gaussian + bilateral kernels, Potts compatibility, symmetric normalisation and iteration count as the pydensecrf calls of the
reference, with every pixel pair summed instead of pydensecrf's permutohedral-lattice approximation (parity
with pydensecrf's own numbers is unpinned).  ``scores_mask_sample_crf`` / ``scores_fake_mask_crf`` (metric.py:79-102) sit on
it.  Left out: ``scores_mask_fake_crf`` (a cubic-spline zoom across the class axis) and ``scores_seg_da_fake``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _abi as A
from . import kernels as K

# metric.py:11-16 -- read at call time, so they can be set on the module as in the reference
MAX_ITER = 10
POS_W = 3
POS_XY_STD = 1
Bi_W = 4
Bi_XY_STD = 67
Bi_RGB_STD = 3


def _labels(x, dev):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(dev).to(torch.int32).contiguous().view(-1)


def _accumulate_hist(hist, label_true, label_pred, n_class):
    """Adds one (true, predicted) label pair to the device-resident int64 confusion matrix ``hist`` (flat n_class^2)."""
    lt, lp = _labels(label_true, hist.device), _labels(label_pred, hist.device)
    assert lt.numel() == lp.numel()
    A.check(A.lib().sgg_confusion_hist(K._p(lt), K._p(lp), lt.numel(), n_class, K._p(hist), K._s()), "confusion_hist")


def _fast_hist(label_true, label_pred, n_class):
    """metric.py:18-24 -- (n_class, n_class) int64 confusion matrix; labels as int arrays/tensors of equal size."""
    hist = torch.zeros(n_class * n_class, dtype=torch.int64, device="cuda")
    _accumulate_hist(hist, label_true, label_pred, n_class)
    return hist.view(n_class, n_class).cpu().numpy()


def scores(label_trues, label_preds, n_class):
    """metric.py:27-47 -- the FCN score set (same keys).  The confusion matrix of ALL pairs is accumulated on the device
    in one int64 buffer (exact, order independent) and read back once; the five scores are then ratios of its
    per-class true-positive / ground-truth / prediction counts."""
    hist = torch.zeros(n_class * n_class, dtype=torch.int64, device="cuda")
    for lt, lp in zip(label_trues, label_preds):
        _accumulate_hist(hist, lt, lp, n_class)
    h = hist.view(n_class, n_class).cpu().numpy()
    tp = np.diagonal(h).astype(np.float64)            # correctly labelled pixels per class
    n_true = h.sum(axis=1).astype(np.float64)         # pixels whose ground truth is the class
    n_pred = h.sum(axis=0).astype(np.float64)         # pixels predicted as the class
    total = float(h.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = tp / (n_true + n_pred - tp)
        seen = n_true > 0
        share = n_true / total
        out = {"Overall Acc": tp.sum() / total,
               "Mean Acc": np.nanmean(tp / n_true),
               "FreqW Acc": (share[share > 0] * iou[share > 0]).sum(),
               "Mean IoU": np.nanmean(iou[seen]),
               "Class IoU": {c: iou[c] for c in range(n_class)}}
    return out


def argmax_u8_labels(img, c_real=None):
    """labels (N,H,W) int32 = argmax over channels of uint8(255*img) -- the label rule of scores_seg_fake.
    img: (N,H,W,C) numpy / torch (float32 real channels, or an internal channel-padded activation with c_real given)."""
    t = img if isinstance(img, torch.Tensor) else torch.as_tensor(np.asarray(img, dtype=np.float32))
    t = t.cuda().contiguous()
    if t.dtype not in (torch.float32, torch.bfloat16):
        t = t.float()
    Cp = t.shape[-1]
    Cr = Cp if c_real is None else c_real
    out = torch.empty(t.shape[:-1], dtype=torch.int32, device=t.device)
    A.check(A.lib().sgg_argmax_u8_labels(K._p(t), K._p(out), out.numel(), Cr, Cp, K.dt(t), K._s()), "argmax_u8_labels")
    return out


def scores_seg_fake(seg_image, fake_img):
    """metric.py:71-77: true labels from seg_image, predicted labels from fake_img; both returned transposed to
    (N, W, H) exactly as ``np.argmax(x.transpose(0,3,2,1), axis=1)`` does."""
    f = fake_img.tensor() if hasattr(fake_img, "tensor") else fake_img
    gts = argmax_u8_labels(seg_image).permute(0, 2, 1).contiguous()
    preds = argmax_u8_labels(f).permute(0, 2, 1).contiguous()
    return gts.cpu().numpy(), preds.cpu().numpy()


def _device(x):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
    return t.cuda()


def dense_crf(img, output_probs):
    """metric.py:49-69: img (h,w,3) uint8, output_probs (c,h,w) -> Q (c,h,w) float32 after MAX_ITER mean-field steps of the
    fully connected CRF (unary -log(clip(p, 1e-5, 1)); Gaussian POS_W / POS_XY_STD; bilateral Bi_W / Bi_XY_STD / Bi_RGB_STD).
    NumPy arrays in -> NumPy array out; device tensors in -> device tensor out."""
    on_device = isinstance(output_probs, torch.Tensor)
    p = _device(output_probs).to(torch.float32).contiguous()
    im = _device(img).to(torch.uint8).contiguous()
    if p.dim() != 3 or tuple(im.shape) != (p.shape[1], p.shape[2], 3):
        raise ValueError(f"dense_crf: image {tuple(im.shape)} does not match probabilities {tuple(p.shape)}")
    q = K.dense_crf(im, probs=p, max_iter=MAX_ITER, pos_w=POS_W, pos_xy_std=POS_XY_STD, bi_w=Bi_W, bi_xy_std=Bi_XY_STD,
                    bi_rgb_std=Bi_RGB_STD)
    return q if on_device else q.cpu().numpy()


def _crf_of_mask(seg_mask_64, rescaled_sample):
    """The shared head of metric.py:79-102: uint8 casts, the mask as (N,C,W,H), dense_crf on sample 0 and the argmax of its
    marginals as (1,W,H).  The reference transposes the mask and not the image; the image's buffer is read as (W,H,3), which is
    the reference's own call when H == W."""
    sample_uint = _device(rescaled_sample).to(torch.uint8)
    mask_uint = _device(seg_mask_64).to(torch.uint8).permute(0, 3, 2, 1).contiguous()
    h, w = mask_uint.shape[2:]
    q = dense_crf(sample_uint[0].contiguous().view(h, w, 3), mask_uint[0])
    return mask_uint, torch.argmax(q, dim=0)[None]


def scores_mask_sample_crf(seg_mask_64, rescaled_sample):
    """metric.py:79-89 -- true labels: the class mask; predicted: dense_crf(sample image, class mask).  seg_mask_64 (N,H,W,C),
    rescaled_sample (N,H,W,3) in 0..255; returns int arrays (N,W,H) and (1,W,H)."""
    mask_uint, crf_probs = _crf_of_mask(seg_mask_64, rescaled_sample)
    crf_labels = torch.argmax(mask_uint, dim=1)
    return crf_labels.cpu().numpy(), crf_probs.cpu().numpy()


def scores_fake_mask_crf(seg_mask_64, rescaled_sample, fake_img):
    """metric.py:92-102 -- true labels: argmax over the channels of uint8(fake_img) (tf.image.convert_image_dtype: a float image
    is scaled and truncated, a uint8 one passes through); predicted: dense_crf(sample image, class mask)."""
    from .utils import convert_image_dtype_uint8
    _, crf_probs = _crf_of_mask(seg_mask_64, rescaled_sample)
    f = fake_img.tensor() if hasattr(fake_img, "tensor") else fake_img
    f = f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
    f_uint = f if f.dtype == np.uint8 else convert_image_dtype_uint8(f).astype(np.uint8)
    crf_labels = np.argmax(f_uint.transpose(0, 3, 2, 1), axis=1)
    return crf_labels, crf_probs.cpu().numpy()
