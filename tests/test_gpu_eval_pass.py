"""The evaluation pass (evaluate.py) with EVERY score on at once: ``test_during_train`` and ``test`` of one cycle model that keeps
a weight average, on the city_small samples at 32 x 32 (square: the CRF; >= 11: SSIM; two SWD levels).

The scores are integer counts, or sums taken in a fixed order, of the 8-bit images: every value must EQUAL what a direct call
of the metric function gives on the fakes the method returned and the same samples.  ``test`` prints with %f: its lines are
compared as the strings those values format to.
"""
import os

import numpy as np
import pytest
import torch

import sggan_amd
from sggan_amd import metric as M
from sggan_amd import segment_class as SC
from sggan_amd.utils import SummarySink, convert_image_dtype_uint8
from tests import class_scores_oracle as O

pytestmark = pytest.mark.gpu

FCN_TAGS = ["Overall Accuracy", "Mean Accuracy", "Frequency Weighted Accuracy", "Mean IoU"]
ALL_TAGS = FCN_TAGS + ["CRF " + t for t in FCN_TAGS] + ["Class " + t for t in FCN_TAGS] + ["Boundary Class Mean IoU"] + \
    ["Class CRF " + t for t in FCN_TAGS] + ["Image MAE", "Image PSNR", "Image SSIM", "Cycle MAE", "Cycle PSNR", "Cycle SSIM"] + \
    ["SWD 32x32", "SWD 16x16", "SWD Mean", "EMA Decay"]
FCN_KEYS = ["Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"]
NO_MASK = "test samples must carry the one-hot class mask (data.directory_test_samples over a DatasetCache(with_class=True))"
N_CLASS, PATCHES, EPOCH = 34, 8, 6


def _args(**kw):
    return sggan_amd.default_args(**dict(dict(ngf=8, ndf=8, n_blocks=2, dtype="f32", image_height=32, image_width=32, dataset_dir=O.FIX,
                                              test_dir=None, cycle=True, ema_decay=0.5), **kw))


ON = dict(crf=True, class_scores=True, boundary_px=3, image_scores=True, swd=True, swd_patches=PATCHES)


def _u8(img01):
    return convert_image_dtype_uint8(np.asarray(img01)[None]).astype(np.uint8)


@pytest.fixture(scope="module")
def done(tmp_path_factory):
    """One model, one ``test_during_train`` with everything on, and the direct metric calls on what it returned."""
    from sggan_amd import data as D
    caches = [D.DatasetCache(O.FIX, split, device="cuda", with_class=True) for split in ("testA", "trainA")]
    samples = [s for c in caches for s in D.directory_test_samples(_args(), c)()]
    assert len(samples) == 3 and all(len(s) == 4 and s[3].shape == (32, 32, N_CLASS) for s in samples)
    palette = SC.learn_palette(caches[0])
    model = sggan_amd.sggan(_args())
    out = str(tmp_path_factory.mktemp("during") / "not_yet_there")
    a = _args(test_dir=out, **ON)
    a.class_palette = palette
    sink = SummarySink()
    fakes, score = model.test_during_train(EPOCH, a, iter(samples), sink)           # (an unsized iterable: SWD needs the count)
    assert fakes.shape == (3, 32, 32, 3) and fakes.dtype == np.uint8

    want = {}
    seg = [M.scores_seg_fake(np.asarray(s[2], dtype=np.float32)[None], torch.as_tensor(fakes[i:i + 1].astype(np.float32))) for i, s in enumerate(samples)]
    want["base"] = M.scores([t for lt, _ in seg for t in lt], [p for _, lp in seg for p in lp], n_class=N_CLASS)
    rescaled = [convert_image_dtype_uint8(np.asarray(s[1])[None]) for s in samples]
    crf = [M.scores_mask_sample_crf(np.asarray(s[3])[None], r) for s, r in zip(samples, rescaled)]
    want["CRF"] = M.scores([t for lt, _ in crf for t in lt], [p for _, lp in crf for p in lp], n_class=N_CLASS)
    truth = [s[3].argmax(axis=-1)[None].astype(np.uint8) for s in samples]
    hists = [None, None, None]
    for i in range(3):
        hists[0] = M.scores_class_fake(truth[i], fakes[i:i + 1], N_CLASS, palette, hist=hists[0])
        hists[1] = M.scores_class_fake(truth[i], fakes[i:i + 1], N_CLASS, palette, band_radius=3, hist=hists[1])
        hists[2] = M.scores_class_fake_crf(truth[i], rescaled[i], fakes[i:i + 1], N_CLASS, palette, hist=hists[2])
    want["Class"], want["Class Boundary"], want["Class CRF"] = (M.scores_from_hist(h) for h in hists)
    image, cycle = [], []
    with model.ema_weights():                                                       # the weights the pass ran on
        for i, s in enumerate(samples):
            M.scores_image_fake(_u8(s[2]), fakes[i:i + 1], image)
            M.scores_image_fake(rescaled[i].astype(np.uint8), model.generator_BA(model.generator(torch.as_tensor(rescaled[i]).to(model.device))), cycle)
    want["Image"], want["Cycle"] = M.scores_from_quality(image), M.scores_from_quality(cycle)
    want["SWD"] = M.sliced_wasserstein(fakes, np.concatenate([_u8(s[2]) for s in samples]), patches=PATCHES)
    want["EMA Decay"] = float(model.generator.P._ema_state[0].item())
    return {"model": model, "args": a, "samples": samples, "palette": palette, "records": sink.records, "fakes": fakes, "score": score,
            "want": want, "out": out}


def test_every_scalar_in_the_documented_order(done):
    assert [r["tag"] for r in done["records"]] == ALL_TAGS and all(r["step"] == EPOCH for r in done["records"])
    assert list(done["score"]) == FCN_KEYS + ["Class IoU", "CRF", "Class", "Class Boundary", "Class CRF", "Image", "Cycle", "SWD"]
    # only <test_dir>/<basename>, in a folder made when the first image was there to write
    assert sorted(os.listdir(done["out"])) == sorted(os.path.basename(s[0]) for s in done["samples"])


def test_every_group_equals_the_direct_metric_calls(done):
    want, score = done["want"], done["score"]
    got = {r["tag"]: r["value"] for r in done["records"]}
    np.testing.assert_equal({k: score[k] for k in FCN_KEYS + ["Class IoU"]}, want["base"])
    for key in ("CRF", "Class", "Class Boundary", "Class CRF", "Image", "Cycle", "SWD"):
        np.testing.assert_equal(score[key], want[key])
    for prefix, s in (("", want["base"]), ("CRF ", want["CRF"]), ("Class ", want["Class"]), ("Class CRF ", want["Class CRF"])):
        assert [got[prefix + t] for t in FCN_TAGS] == [float(s[k]) for k in FCN_KEYS], prefix
    assert got["Boundary Class Mean IoU"] == float(want["Class Boundary"]["Mean IoU"])
    for key in ("Image", "Cycle"):
        assert [got[key + " " + q] for q in ("MAE", "PSNR", "SSIM")] == [want[key][q] for q in ("MAE", "PSNR", "SSIM")], key
    assert [got[t] for t in ("SWD 32x32", "SWD 16x16", "SWD Mean")] == [v for _, _, v in want["SWD"]["levels"]] + [want["SWD"]["mean"]]
    assert [(h, w) for h, w, _ in want["SWD"]["levels"]] == [(32, 32), (16, 16)] and want["SWD"]["mean"] > 0
    assert got["EMA Decay"] == want["EMA Decay"]
    assert want["Image"]["MAE"] > 0 and want["Cycle"]["MAE"] > 0 and want["Image"]["MAE"] != want["Cycle"]["MAE"]


@pytest.mark.parametrize("options,message", [(ON, "crf: " + NO_MASK), (dict(ON, crf=False), "class_scores: " + NO_MASK)])
def test_samples_without_the_class_mask_raise_before_any_scalar(done, options, message):
    a = _args(**options)
    a.class_palette = done["palette"]
    sink = SummarySink()
    with pytest.raises(ValueError) as e:
        done["model"].test_during_train(EPOCH, a, [s[:3] for s in done["samples"]], sink)
    assert str(e.value) == message and sink.records == []


def test_phase_test_logs_the_same_values_and_writes_both_files(done, tmp_path):
    want, names = done["want"], [os.path.basename(s[0]) for s in done["samples"]]
    a = _args(test_dir=str(tmp_path / "out"), checkpoint_dir=str(tmp_path / "ckpt"), **ON)
    a.class_palette = done["palette"]
    lines = []
    outs = done["model"].test(a, iter(done["samples"]), log=lines.append)
    assert len(outs) == 3 and sorted(os.listdir(a.test_dir)) == sorted(names + ["real_" + n for n in names])
    assert lines[:2] == [" [*] Running Test ...", " [!] Load failed..."] and lines[2:5] == ["Processing image: " + n for n in names]
    c, q, w = want["Class"], want["Image"], want["SWD"]
    assert lines[5:] == [
        "Class Overall Accuracy: %f Class Mean Accuracy: %f Class Frequency Weighted Accuracy: %f Class Mean IoU: %f"
        % (c["Overall Acc"], c["Mean Acc"], c["FreqW Acc"], c["Mean IoU"]),
        "Image MAE: %f Image PSNR: %f Image SSIM: %f" % (q["MAE"], q["PSNR"], q["SSIM"]),
        "SWD 32x32: %f SWD 16x16: %f SWD Mean: %f" % (w["levels"][0][2], w["levels"][1][2], w["mean"])]
    # samples of two elements: nothing to score, no summary line, no error
    bare = []
    done["model"].test(a, [s[:2] for s in done["samples"]], log=bare.append)
    assert bare == lines[:5]
