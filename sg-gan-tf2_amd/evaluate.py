"""The evaluation pass behind ``sggan.test_during_train`` and ``sggan.test``: ``run`` hands every translated ``Sample``
to the scorers, one per score family.  A scorer has ``add(sample)``; ``result(strict)``, its entries of the score dict (the ONE
read-back of its device-side sums) or None; ``scalars(result)``; ``needs`` elements per sample, else a strict pass raises ``missing``."""
from __future__ import annotations

from functools import cached_property

import numpy as np
import torch

from . import metric as M
from .utils import convert_image_dtype_uint8, get_img

FCN = (("Overall Accuracy", "Overall Acc"), ("Mean Accuracy", "Mean Acc"), ("Frequency Weighted Accuracy", "FreqW Acc"), ("Mean IoU", "Mean IoU"))
QUALITY = (("MAE", "MAE"), ("PSNR", "PSNR"), ("SSIM", "SSIM"))
# the order of the scalars after the reference's four: (key of the score set in the score dict, prefix of the names, (name, key) pairs)
SETS = (("CRF", "CRF ", FCN), ("Class", "Class ", FCN), ("Class Boundary", "Boundary Class ", FCN[3:]), ("Class CRF", "Class CRF ", FCN),
        ("Image", "Image ", QUALITY), ("Cycle", "Cycle ", QUALITY))
NO_MASK = "test samples must carry the one-hot class mask (data.directory_test_samples over a DatasetCache(with_class=True))"


def scalars(res, ema_decay=None):
    """The (tag, value) pairs of the score sets in ``res`` (one scorer's result, or the whole score dict) in the order a sink gets them: the
    reference's four (model.py:389-393), ``SETS``, 'SWD <h>x<w>' per level, finest first, 'SWD Mean', 'EMA Decay'  where given."""
    out = [(tag, res[key]) for tag, key in FCN if key in res]
    for key, prefix, fields in SETS:
        if key in res:
            out += [(prefix + tag, res[key][field]) for tag, field in fields]
    if "SWD" in res:
        out += [("SWD %dx%d" % (h, w), v) for h, w, v in res["SWD"]["levels"]] + [("SWD Mean", res["SWD"]["mean"])]
    return out + ([("EMA Decay", ema_decay)] if ema_decay is not None else [])


class Sample:
    """One test sample (name, image (H,W,3) in [0,1][, label image (H,W,3) in [0,1][, one-hot class mask (H,W,C)]]): ``rescaled`` is the
    image as the reference feeds it (convert_image_dtype -> uint8 -> float32, model.py:352-353), ``fake`` the generator's lazy output
    for it (:357), ``total`` the number of samples where known.  The rest is made on first use, once."""
    def __init__(self, item, generator, device, total):
        self.item, self.device, self.total, self.name, self.image = item, device, total, item[0], np.asarray(item[1], dtype=np.float32)
        self.has_label, self.has_mask = len(item) >= 3, len(item) >= 4
        self.rescaled = convert_image_dtype_uint8(self.image[None])
        self.fake = generator(torch.as_tensor(self.rescaled).to(device))

    @cached_property
    def fake_img(self):         # the translation as the (1,H,W,3) uint8 image save_images writes (model.py:369)
        return get_img(self.fake, [1, 1])

    @cached_property
    def label_u8(self):         # the label image as 8-bit colours (1,H,W,3)
        return convert_image_dtype_uint8(np.asarray(self.item[2])[None]).astype(np.uint8)

    @cached_property
    def truth(self):            # the ground-truth class map (1,H,W) uint8, on the device
        return torch.argmax(torch.as_tensor(np.asarray(self.item[3])).to(self.device), dim=-1).to(torch.uint8)[None]


class Scorer:
    needs, missing, scalars = 3, "test samples must carry their label image as the third element", staticmethod(scalars)


class SegLabels(Scorer):
    """The reference's scores (model.py:373-393): every translation is labelled against its label image (metric.scores_seg_fake);
    the FCN scores of all labels (metric.scores) are the top level of the score dict and go out under the reference's names."""
    def __init__(self, n_class):
        self.n_class, self.gts, self.preds = n_class, [], []

    def add(self, s):
        lt, lp = M.scores_seg_fake(np.asarray(s.item[2], dtype=np.float32)[None], torch.as_tensor(s.fake_img.astype(np.float32)))   # :373
        self.gts.extend(lt)
        self.preds.extend(lp)

    def result(self, strict):
        return M.scores(self.gts, self.preds, n_class=self.n_class)                                                               # :378


class CrfLabels(SegLabels):
    """``args.crf``: the sample's one-hot class mask against dense_crf(sample image, mask) (metric.scores_mask_sample_crf;
    model.py:314-315,330,338 keep the lists for it): "CRF", 'CRF Overall Accuracy' ... 'CRF Mean IoU'."""
    needs, missing = 4, "crf: " + NO_MASK

    def add(self, s):
        lt, lp = M.scores_mask_sample_crf(np.asarray(s.item[3])[None], s.rescaled)
        self.gts.extend(lt)
        self.preds.extend(lp)

    def result(self, strict):
        return {"CRF": super().result(strict)}


class ClassHists(Scorer):
    """``args.class_scores``: the argmax of the class mask is the ground truth, the translation is decoded to classes
    through ``args.class_palette`` (segment_class.learn_palette; None: the built-in table), ONE confusion matrix per score set is
    accumulated on the device.  "Class": the four 'Class ...'; ``band_px`` > 0, "Class Boundary", the pixels within that distance of a
    ground-truth class boundary: 'Boundary Class Mean IoU'; ``crf``, "Class CRF", the CRF-refined map (metric.scores_class_fake_crf)."""
    needs, missing = 4, "class_scores: " + NO_MASK

    def __init__(self, args, device, band_px=0, crf=False):
        far = int(getattr(args, "class_max_dist", -1))
        self.band_px, self.count = band_px, 0
        self.kw = dict(n_class=args.segment_class, palette=getattr(args, "class_palette", None), max_dist2=far * far if far >= 0 else -1)
        self.hist = {k: torch.zeros((args.segment_class,) * 2, dtype=torch.int64, device=device)
                     for k, on in (("Class", True), ("Class Boundary", band_px > 0), ("Class CRF", crf)) if on}

    def add(self, s):
        if s.has_mask:
            self.count += 1
            M.scores_class_fake(s.truth, s.fake, hist=self.hist["Class"], **self.kw)
            if "Class Boundary" in self.hist:
                M.scores_class_fake(s.truth, s.fake, band_radius=self.band_px, hist=self.hist["Class Boundary"], **self.kw)
            if "Class CRF" in self.hist:
                M.scores_class_fake_crf(s.truth, s.rescaled, s.fake, hist=self.hist["Class CRF"], **self.kw)

    def result(self, strict):   # a strict pass reports its matrices even over no sample at all
        return {k: M.scores_from_hist(h) for k, h in self.hist.items()} if strict or self.count else None


class ImageQuality(Scorer):
    """``args.image_scores``: every translation, as the 8-bit image ``save_images`` writes, against the 8-bit label image
    (metric.scores_image_fake): "Image"; a cycle model's ``generator_BA(fake)``, under the same weights, against the 8-bit input: "Cycle"."""
    def __init__(self, generator_BA=None):
        self.generator_BA, self.acc = generator_BA, {"Image": [], "Cycle": []}

    def add(self, s):
        if s.has_label:
            M.scores_image_fake(s.label_u8, s.fake, self.acc["Image"])
        if self.generator_BA is not None:
            M.scores_image_fake(s.rescaled.astype(np.uint8), self.generator_BA(s.fake), self.acc["Cycle"])

    def result(self, strict):
        return {k: M.scores_from_quality(a) for k, a in self.acc.items() if a} or None


class Swd(Scorer):
    """``args.swd``: every translation goes, as that 8-bit image, into the fakes of a metric.SWD (``args.swd_patches``
    descriptors per level and image).  The reals are the samples' own 8-bit label images, or, where ``reals`` is given, the (H,W,3) images
    in [0,1] it yields (a callable is called first) -- an unpaired set, of which as many are used as there are fakes.  "SWD"."""
    def __init__(self, model, args, reals):
        self.model, self.patches, self.reals, self.swd = model, int(getattr(args, "swd_patches", 128)), reals, None
        self.needs = 3 if reals is None else 2

    def add(self, s):
        if self.swd is None:    # the set-wide descriptor buffers are sized once, from the number of samples
            self.swd = M.SWD(self.model.image_height, self.model.image_width, s.total, patches=self.patches, device=self.model.device)
        self.swd.add_fakes(s.fake)
        if self.reals is None and s.has_label:
            self.swd.add_reals(s.label_u8)

    def result(self, strict):   # a strict pass without reals is metric.SWD's error; otherwise there is no result
        if self.swd is not None:
            if self.reals is not None:
                swd_add_reals(self.swd, self.reals)
            if strict or self.swd.count["reals"]:
                return {"SWD": self.swd.result()}


def swd_add_reals(swd, swd_reals):
    """The unpaired reals of a test pass: (H,W,3) images in [0,1], as many as there are fakes."""
    for img in (swd_reals() if callable(swd_reals) else swd_reals):
        if swd.count["reals"] >= swd.count["fakes"]:
            break
        swd.add_reals(convert_image_dtype_uint8(np.asarray(img)[None]).astype(np.uint8))


def run(model, samples, scorers, each, strict):
    """The pass: under the weights the test passes run on (the moving average, where kept), per sample ONE generator call, ``each(sample)``
    -- the caller's saving and logging --, then every scorer in the order given.  ``strict``: a sample with fewer elements than a scorer needs
    is that scorer's ValueError, before anything is done with it; else the scorer skips it.  Returns (``each``'s outputs, the results there are)."""
    if any(isinstance(sc, Swd) for sc in scorers) and not hasattr(samples, "__len__"):
        samples = list(samples)
    outputs = []
    with model._test_weights():
        for item in samples:
            for sc in scorers:
                if strict and len(item) < sc.needs:
                    raise ValueError(sc.missing)
            s = Sample(item, model.generator, model.device, len(samples) if hasattr(samples, "__len__") else None)
            outputs.append(each(s))
            for sc in scorers:
                sc.add(s)
    return outputs, [res for res in (sc.result(strict) for sc in scorers) if res is not None]
