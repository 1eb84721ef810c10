"""The reporting layer of the evaluation pass (evaluate.py) without a device: the order of the scalars, spelled out, from canned
results; and ``metric.scores_from_hist`` against the closed form of one hand-written confusion matrix."""
import itertools

import numpy as np
import torch

from sggan_amd import evaluate as E
from sggan_amd import metric as M

FCN = {"Overall Acc": 0.5, "Mean Acc": 0.25, "FreqW Acc": 0.125, "Mean IoU": 0.0625, "Class IoU": {0: 1.0}}
QUALITY = {"MAE": 3.0, "PSNR": 20.0, "SSIM": 0.5, "per_image": {}}


def _shifted(d, by):
    return {k: (v + by if isinstance(v, float) else v) for k, v in d.items()}


# (scorer, the result it reports, the tags of that result) per group of the documented order
GROUPS = [
    (E.SegLabels, FCN, ["Overall Accuracy", "Mean Accuracy", "Frequency Weighted Accuracy", "Mean IoU"]),
    (E.CrfLabels, {"CRF": _shifted(FCN, 1.0)}, ["CRF Overall Accuracy", "CRF Mean Accuracy", "CRF Frequency Weighted Accuracy", "CRF Mean IoU"]),
    (E.ClassHists, {"Class": _shifted(FCN, 2.0), "Class Boundary": _shifted(FCN, 3.0), "Class CRF": _shifted(FCN, 4.0)},
     ["Class Overall Accuracy", "Class Mean Accuracy", "Class Frequency Weighted Accuracy", "Class Mean IoU", "Boundary Class Mean IoU",
      "Class CRF Overall Accuracy", "Class CRF Mean Accuracy", "Class CRF Frequency Weighted Accuracy", "Class CRF Mean IoU"]),
    (E.ImageQuality, {"Image": QUALITY, "Cycle": _shifted(QUALITY, 1.0)},
     ["Image MAE", "Image PSNR", "Image SSIM", "Cycle MAE", "Cycle PSNR", "Cycle SSIM"]),
    (E.Swd, {"SWD": {"levels": [(32, 32, 7.0), (16, 16, 8.0)], "mean": 7.5}}, ["SWD 32x32", "SWD 16x16", "SWD Mean"]),
]
EVERYTHING = [
    ("Overall Accuracy", 0.5), ("Mean Accuracy", 0.25), ("Frequency Weighted Accuracy", 0.125), ("Mean IoU", 0.0625),
    ("CRF Overall Accuracy", 1.5), ("CRF Mean Accuracy", 1.25), ("CRF Frequency Weighted Accuracy", 1.125), ("CRF Mean IoU", 1.0625),
    ("Class Overall Accuracy", 2.5), ("Class Mean Accuracy", 2.25), ("Class Frequency Weighted Accuracy", 2.125), ("Class Mean IoU", 2.0625),
    ("Boundary Class Mean IoU", 3.0625),
    ("Class CRF Overall Accuracy", 4.5), ("Class CRF Mean Accuracy", 4.25), ("Class CRF Frequency Weighted Accuracy", 4.125),
    ("Class CRF Mean IoU", 4.0625),
    ("Image MAE", 3.0), ("Image PSNR", 20.0), ("Image SSIM", 0.5),
    ("Cycle MAE", 4.0), ("Cycle PSNR", 21.0), ("Cycle SSIM", 1.5),
    ("SWD 32x32", 7.0), ("SWD 16x16", 8.0), ("SWD Mean", 7.5),
    ("EMA Decay", 0.75),
]


def _merged(groups):
    return {k: v for _, res, _ in groups for k, v in res.items()}


def test_the_scalars_of_every_scorer_in_the_documented_order():
    assert [tv for sc, res, _ in GROUPS for tv in sc.scalars(res)] == EVERYTHING[:-1]        # scorer by scorer, as sggan.test logs them
    for sc, res, tags in GROUPS:
        assert [t for t, _ in sc.scalars(res)] == tags
    assert E.scalars(_merged(GROUPS), 0.75) == EVERYTHING                                   # the score dict, as test_during_train writes it
    assert E.scalars(_merged(GROUPS)) == EVERYTHING[:-1]                                    # a model without a weight average
    assert E.scalars(_merged(reversed(GROUPS)), 0.75) == EVERYTHING                         # (the order is the table's, not the dict's)


def test_absent_groups_leave_the_rest_in_their_order():
    for keep in itertools.product((False, True), repeat=len(GROUPS)):
        kept = [g for g, k in zip(GROUPS, keep) if k]
        tags = {t for _, _, ts in kept for t in ts} | {"EMA Decay"}
        assert E.scalars(_merged(kept), 0.75) == [tv for tv in EVERYTHING if tv[0] in tags], keep
    # within a scorer: the score sets its options leave out
    part = lambda sc, res, keys: [t for t, _ in sc.scalars({k: res[k] for k in keys})]
    _, classes, class_tags = GROUPS[2]
    assert part(E.ClassHists, classes, ["Class"]) == class_tags[:4]                      # boundary_px = 0, no crf
    assert part(E.ClassHists, classes, ["Class", "Class Boundary"]) == class_tags[:5]
    assert part(E.ClassHists, classes, ["Class", "Class CRF"]) == class_tags[:4] + class_tags[5:]
    assert part(E.ImageQuality, GROUPS[3][1], ["Image"]) == GROUPS[3][2][:3]             # not a cycle model


def test_scores_from_hist_is_the_closed_form_of_a_hand_written_matrix():
    """Rows: ground truth, columns: prediction.  Class 2 is predicted once and never the ground truth: its accuracy is 0/0
    (left out by the nanmean), its IoU 0/1 = 0 (left out of the mean by the ``seen`` mask, which is why that mean is 1/2, not 1/3)."""
    h = np.array([[3, 1, 1],
                  [2, 4, 0],
                  [0, 0, 0]], dtype=np.int64)
    want = {"Overall Acc": 7 / 11, "Mean Acc": (3 / 5 + 4 / 6) / 2, "FreqW Acc": 5 / 11 * (3 / 7) + 6 / 11 * (4 / 7), "Mean IoU": (3 / 7 + 4 / 7) / 2}
    for form in (h, h.reshape(-1), torch.as_tensor(h), torch.as_tensor(h).view(-1)):
        got = M.scores_from_hist(form)
        assert set(got) == set(want) | {"Class IoU"}
        for k, v in want.items():
            assert abs(got[k] - v) <= 4e-16, (k, got[k], v)         # values below 1 (ulp 1.1e-16), at most three roundings on either side
        assert got["Class IoU"] == {0: 3 / 7, 1: 4 / 7, 2: 0.0}
    # a class that is neither: its IoU is 0/0, and every mean leaves it out
    h4 = np.zeros((4, 4), dtype=np.int64)
    h4[:3, :3] = h
    got = M.scores_from_hist(h4)
    assert np.isnan(got["Class IoU"][3]) and got["Class IoU"][2] == 0.0
    for k, v in want.items():
        assert abs(got[k] - v) <= 4e-16, (k, got[k], v)
