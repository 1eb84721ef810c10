"""Evaluation metrics -- mirror of the NumPy part of the reference's ``metric.py`` (next-row SURVEY.md 8(f)4).

``_fast_hist`` / ``scores`` (metric.py:18-47) with the confusion matrix accumulated on the GPU (integer atomics:
exact and order-independent) and ``scores_seg_fake`` (metric.py:71-77).

``dense_crf`` (metric.py:49-69) runs on the GPU as an EXACT mean-field fully connected CRF (csrc/crf.hip): the same unary,
Gaussian + bilateral kernels, Potts compatibility, symmetric normalisation and iteration count as the pydensecrf calls of the
reference, with every pixel pair summed instead of pydensecrf's permutohedral-lattice approximation (parity
with pydensecrf's own numbers is unpinned).  ``scores_mask_sample_crf`` / ``scores_fake_mask_crf`` (metric.py:79-102) sit on
it.  ``scores_mask_fake_crf`` (a cubic-spline zoom across the class axis) is superseded by ``scores_class_fake_crf``;
``scores_seg_da_fake`` is left out.

Class-level scores (not in the reference): ``palette_labels`` / ``palette_probs`` decode a generated colour map
to classes through a palette learned from the dataset (csrc/evalseg.hip), ``scores_class_fake`` counts it against the class
map in the same launch (optionally on a boundary band), ``scores_class_fake_crf`` refines it with ``dense_crf`` first.

Paired image quality (not in the reference): ``image_quality`` gives the mean absolute error, MSE, PSNR and SSIM
(Wang et al.; 11 x 11 Gaussian window, sigma 1.5, data range 255, the mean over the windows inside the image) of two images
taken as 8-bit colours -- the bytes ``save_images`` writes -- from integer sums and a double-precision SSIM map summed in a
fixed order on the GPU (csrc/imgqual.hip).  ``scores_image_fake`` keeps the per-image sums of a test pass on the device,
``scores_from_quality`` reads them back once and pools them.

Unpaired realism (not in the reference): ``SWD`` / ``sliced_wasserstein`` give the sliced Wasserstein distance of
Laplacian-pyramid patches (Karras et al. 2018) between a set of fakes and a set of reals, taken as 8-bit colours: pyramid, patch
gather, normalise-and-project and distance on the GPU (csrc/swd.hip), the sort by ``torch.sort``, one read-back.
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
    """metric.py:27-47 -- the FCN score set: ONE int64 confusion matrix of ALL pairs on the device (exact), read back by ``scores_from_hist``."""
    hist = torch.zeros(n_class * n_class, dtype=torch.int64, device="cuda")
    for lt, lp in zip(label_trues, label_preds):
        _accumulate_hist(hist, lt, lp, n_class)
    return scores_from_hist(hist)


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


# ----------------------------------------------------------------------------- class-level scores (csrc/evalseg.hip)
def _image_tensor(img):
    """A generated image as a device tensor (N,H,W,C): a lazy generator output, a torch tensor or a NumPy array (float in
    [-1,1] -- bf16 / f32 -- or uint8, e.g. the PNG ``save_images`` wrote)."""
    t = img.tensor() if hasattr(img, "tensor") else img
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.array(t))      # (a copy: a decoded PNG is read-only)
    t = t.cuda()
    if t.dim() == 3:
        t = t[None]
    if t.dtype not in (torch.float32, torch.bfloat16, torch.uint8):
        t = t.float()
    return t.contiguous()


def _class_tensor(class_map):
    t = class_map if isinstance(class_map, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(class_map))
    t = t.cuda().to(torch.uint8)
    return (t[None] if t.dim() == 2 else t).contiguous()


def palette_labels(img, palette=None, other_class=0, max_dist2=-1):
    """Class labels int32 (N,H,W), on the device, of a generated colour image: the class of the nearest palette colour (squared
    RGB distance of the 8-bit colours, ties to the lowest entry), ``other_class`` where that distance exceeds ``max_dist2 >= 0``.
    ``palette``: ``(keys, classes)`` from segment_class.learn_palette; None: the built-in table (segment_class.palette)."""
    return K.palette_decode(_image_tensor(img), palette, other_class, max_dist2)[0]


def palette_probs(img, n_class, palette=None, sigma=32.0, other_class=0, max_dist2=-1):
    """Class probabilities f32 (N,n_class,H,W), on the device, of a generated colour image: a softmax over the classes of
    -(smallest squared distance to a colour of the class) / (2 sigma^2); classes without a colour get 0.  Each image's slice
    is what ``dense_crf`` takes as ``output_probs``."""
    return K.palette_probs(_image_tensor(img), n_class, palette, sigma, other_class, max_dist2)


def scores_from_hist(hist):
    """metric.py:27-47 -- the FCN score set (five keys) from a confusion matrix (n_class, n_class) or its flat form, tensor (ONE read-back) or array."""
    h = hist.cpu().numpy() if isinstance(hist, torch.Tensor) else np.asarray(hist)
    n_class = int(round(np.sqrt(h.size)))
    h = h.reshape(n_class, n_class)
    tp = np.diagonal(h).astype(np.float64)            # correctly labelled pixels per class
    n_true = h.sum(axis=1).astype(np.float64)         # pixels whose ground truth is the class
    n_pred = h.sum(axis=0).astype(np.float64)         # pixels predicted as the class
    total = float(h.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = tp / (n_true + n_pred - tp)
        seen = n_true > 0
        share = n_true / total
        return {"Overall Acc": tp.sum() / total,
                "Mean Acc": np.nanmean(tp / n_true),
                "FreqW Acc": (share[share > 0] * iou[share > 0]).sum(),
                "Mean IoU": np.nanmean(iou[seen]),
                "Class IoU": {c: iou[c] for c in range(n_class)}}


def _new_hist(n_class, hist):
    return torch.zeros((n_class, n_class), dtype=torch.int64, device="cuda") if hist is None else hist


def scores_class_fake(class_map, fake_img, n_class, palette, band_radius=0, hist=None, other_class=0, max_dist2=-1):
    """Confusion matrix int64 (n_class, n_class), on the device, of the ground-truth class map (N,H,W) against the palette
    labels of ``fake_img`` -- decode and count fused in one launch.  ``band_radius > 0`` counts only the pixels within that many
    pixels of a class boundary of the ground truth (one more launch).  ``hist``: a matrix to add into (accumulation over a test
    set); feed the result to ``scores_from_hist``."""
    truth, img = _class_tensor(class_map), _image_tensor(fake_img)
    hist = _new_hist(n_class, hist)
    select = K.class_boundary_band(truth, band_radius) if band_radius > 0 else None
    K.palette_decode(img, palette, other_class, max_dist2, truth=truth, select=select, n_class=n_class, hist=hist, want_labels=False)
    return hist


def scores_class_fake_crf(class_map, rescaled_sample, fake_img, n_class, palette, hist=None, other_class=0, max_dist2=-1):
    """As ``scores_class_fake`` with the generated map refined by the photo first: per image the labels are
    ``argmax(dense_crf(photo, palette_probs(fake)))`` (``rescaled_sample`` (N,H,W,3) in 0..255, the MAX_ITER ... Bi_RGB_STD
    constants of this module as they are at call time), counted against the class map by ``sgg_confusion_hist``."""
    truth, img = _class_tensor(class_map), _image_tensor(fake_img)
    photo = _device(rescaled_sample).to(torch.uint8)
    photo = (photo[None] if photo.dim() == 3 else photo).contiguous()
    hist = _new_hist(n_class, hist)
    probs = palette_probs(img, n_class, palette, other_class=other_class, max_dist2=max_dist2)
    for n in range(img.shape[0]):
        labels = torch.argmax(dense_crf(photo[n], probs[n]), dim=0)
        _accumulate_hist(hist.view(-1), truth[n], labels, n_class)
    return hist


# ----------------------------------------------------------------------------- paired image quality (csrc/imgqual.hip)
def _quality_counts(H, W):
    """(values the two integer sums run over, values of the SSIM map) per image."""
    return 3 * H * W, 3 * (H - 10) * (W - 10)


def _per_image_quality(rows, n_all, n_valid):
    """The derived scores of (N,3) sums; n_all / n_valid: scalars or per-row arrays."""
    mse = rows[:, 1] / n_all
    psnr = np.full(len(rows), np.inf)
    psnr[mse > 0] = 10.0 * np.log10(255.0 ** 2 / mse[mse > 0])
    return {"MAE": rows[:, 0] / n_all, "MSE": mse, "PSNR": psnr, "SSIM": rows[:, 2] / n_valid}


def image_quality(a, b):
    """Per-image arrays {"MAE", "MSE", "PSNR", "SSIM"} (float64, NumPy) of two images (N,H,W,C) or (H,W,C), NumPy or torch:
    uint8 with C = 3 | 4, float in [-1,1] (quantised as utils.inverse_transform does), or what the generators return (the
    internal channel-padded activations, a lazy output).  MAE = sum |a-b| / (3HW), MSE = sum (a-b)^2 / (3HW), PSNR =
    10 log10(255^2 / MSE) (inf where MSE is 0), SSIM = the mean of the SSIM map over the (H-10)(W-10) windows inside the image
    and the three channels.  H, W >= 11."""
    ta, tb = _image_tensor(a), _image_tensor(b)
    rows = K.image_quality(ta, tb).cpu().numpy()
    return _per_image_quality(rows, *_quality_counts(ta.shape[1], ta.shape[2]))


def scores_image_fake(target_u8, fake_img, acc=None):
    """Appends the raw (N,3) device rows {sum |a-b|, sum (a-b)^2, SSIM sum} of ``fake_img`` against ``target_u8`` and their
    value counts to ``acc`` (a list; a new one when None) and returns it: nothing is read back, so a test pass collects every
    sample and hands the list to ``scores_from_quality`` once at its end."""
    acc = [] if acc is None else acc
    target, fake = _image_tensor(target_u8), _image_tensor(fake_img)
    acc.append((K.image_quality(target, fake), _quality_counts(target.shape[1], target.shape[2])))
    return acc


def scores_from_quality(acc):
    """{"MAE", "PSNR", "SSIM", "per_image": {"MAE", "MSE", "PSNR", "SSIM"}} of the rows ``scores_image_fake`` collected (ONE
    read-back).  MAE is pooled over all values; PSNR comes from the pooled MSE -- where that is 0, the finite bound
    10 log10(255^2 * count), the PSNR of a single unit error among ``count`` values, so that a JSON sink never holds inf;
    SSIM is the mean of the per-image SSIMs."""
    if not acc:
        raise ValueError("scores_from_quality: no image pair was scored")
    rows = torch.cat([r for r, _ in acc]).cpu().numpy()
    n_all = np.concatenate([np.full(len(r), c[0], dtype=np.float64) for r, c in acc])
    n_valid = np.concatenate([np.full(len(r), c[1], dtype=np.float64) for r, c in acc])
    per = _per_image_quality(rows, n_all, n_valid)
    count = float(n_all.sum())
    pooled_mse = float(rows[:, 1].sum()) / count
    psnr = 10.0 * np.log10(255.0 ** 2 / pooled_mse) if pooled_mse > 0 else 10.0 * np.log10(255.0 ** 2 * count)
    return {"MAE": float(rows[:, 0].sum()) / count, "PSNR": float(psnr), "SSIM": float(np.mean(per["SSIM"])), "per_image": per}


# ----------------------------------------------------------------------------- sliced Wasserstein distance (csrc/swd.hip)
def swd_directions(D, seed=19):
    """The (147, D) float32 projection matrix: Gaussian columns from a seeded host generator, scaled to unit length in double."""
    g = torch.randn((K.SWD_K, int(D)), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64)
    return (g / g.norm(dim=0, keepdim=True)).to(torch.float32).contiguous()


class SWD:
    """Sliced Wasserstein distance of Laplacian-pyramid patches between a set of fakes and a set of reals of H x W, up to
    ``n_max`` images each, taken as the 8-bit colours ``save_images`` writes.  Per level and image ``patches`` 7x7x3 descriptors
    at positions keyed by (seed, image index, level, patch) -- image g of either set gets the same positions --, per set and
    level normalised per colour channel, projected on ``repeats * dirs_per_repeat`` unit directions, sorted, and compared:
    1e3 * mean |a_sorted - b_sorted|.  ``levels``: None takes kernels.swd_default_levels(H, W).  The descriptors of both sets
    stay on the device; ``result`` reads back once."""

    def __init__(self, H, W, n_max, patches=128, repeats=4, dirs_per_repeat=128, seed=19, levels=None, device="cuda"):
        self.H, self.W, self.n_max, self.patches = int(H), int(W), int(n_max), int(patches)
        self.levels = K.swd_default_levels(self.H, self.W) if levels is None else int(levels)
        if self.levels == 0:
            raise ValueError(f"SWD: {self.H}x{self.W} is too small: the level count is the largest L <= {K.SWD_MAX_LEVELS} for which H and W "
                             "divide by 2^(L-1) and min(H, W) >> (L-1) >= 16, and the coarsest level must hold a 7x7 patch")
        if K.swd_pyramid_elems(self.H, self.W, self.levels) == 0:
            raise ValueError(f"SWD: {self.levels} levels at {self.H}x{self.W} are not supported (1..{K.SWD_MAX_LEVELS} levels, H and W "
                             "divisible by 2^(levels-1), a coarsest level of at least 7x7, H*W <= 2^22)")
        if self.n_max <= 0 or self.patches <= 0 or repeats <= 0 or dirs_per_repeat <= 0:
            raise ValueError("SWD: n_max, patches, repeats and dirs_per_repeat must be positive")
        self.seed, self.repeats, self.dirs_per_repeat = int(seed), int(repeats), int(dirs_per_repeat)
        self.device = torch.device(device)
        self.sizes = [(self.H >> l, self.W >> l) for l in range(self.levels)]
        self.directions = swd_directions(self.repeats * self.dirs_per_repeat, self.seed)
        # one contiguous (147, dirs_per_repeat) matrix per repeat: a repeat's projections are sorted on their own
        self._dirs = [self.directions[:, r * self.dirs_per_repeat:(r + 1) * self.dirs_per_repeat].contiguous().to(self.device)
                      for r in range(self.repeats)]
        rows = self.n_max * self.patches
        self._desc = {k: [torch.empty((rows, K.SWD_K), dtype=torch.float32, device=self.device) for _ in range(self.levels)]
                      for k in ("fakes", "reals")}
        self.count = {"fakes": 0, "reals": 0}

    def _add(self, which, imgs):
        t = _image_tensor(imgs).to(self.device)
        N = t.shape[0]
        if tuple(t.shape[1:3]) != (self.H, self.W):
            raise ValueError(f"SWD: image {tuple(t.shape)} where {self.H}x{self.W} was announced")
        at = self.count[which]
        if at + N > self.n_max:
            raise ValueError(f"SWD: more than n_max = {self.n_max} {which}")
        pyr = K.swd_pyramid(t, self.levels)
        P = self.patches
        for l in range(self.levels):
            K.swd_descriptors(pyr, self.H, self.W, self.levels, l, P, self.seed, at, self._desc[which][l][at * P:(at + N) * P])
        self.count[which] = at + N

    def add_fakes(self, imgs):
        self._add("fakes", imgs)

    def add_reals(self, imgs):
        self._add("reals", imgs)

    def add(self, fakes, reals):
        self._add("fakes", fakes)
        self._add("reals", reals)

    def result(self):
        """{"levels": [(h, w, value) ...] finest first, "mean": value} over the first min(fakes, reals) images of both sets."""
        import math
        n = min(self.count.values())
        if n == 0:
            raise ValueError("SWD: a set is empty")
        M, dpr = n * self.patches, self.dirs_per_repeat
        D = self.repeats * dpr
        sums = torch.empty((self.levels, D), dtype=torch.float64, device=self.device)
        pa, pb = (torch.empty((dpr, M), dtype=torch.float64, device=self.device) for _ in range(2))
        mom = torch.empty((3, 2), dtype=torch.float64, device=self.device)
        for l in range(self.levels):
            a, b = self._desc["fakes"][l][:M], self._desc["reals"][l][:M]
            for r, dirs in enumerate(self._dirs):
                K.swd_project(a, dirs, pa, mom)
                K.swd_project(b, dirs, pb, mom)
                K.swd_distance(torch.sort(pa, dim=1).values, torch.sort(pb, dim=1).values, sums[l, r * dpr:(r + 1) * dpr])
        host = sums.cpu().numpy()                                            # the one read-back
        values = [1e3 * math.fsum(host[l]) / (float(D) * float(M)) for l in range(self.levels)]
        return {"levels": [(h, w, v) for (h, w), v in zip(self.sizes, values)], "mean": math.fsum(values) / len(values)}


def sliced_wasserstein(fakes, reals, batch=16, **kw):
    """The one-shot form of ``SWD``: two image sets (N,H,W,C) as ``SWD.add`` takes them -> ``SWD.result()``."""
    shape = lambda x: tuple(x.tensor().shape if hasattr(x, "tensor") else x.shape)
    (nf, H, W), nr = shape(fakes)[:3], shape(reals)[0]
    s = SWD(H, W, max(nf, nr), **kw)
    for which, imgs, n in (("fakes", fakes, nf), ("reals", reals, nr)):
        imgs = imgs.tensor() if hasattr(imgs, "tensor") else imgs
        for i in range(0, n, batch):
            s._add(which, imgs[i:i + batch])
    return s.result()
