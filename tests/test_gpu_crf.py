"""metric.dense_crf on the GPU (csrc/crf.hip) against the float64 oracle of tests/crf_oracle.py.

Bounds.  eps32 (tests/golden/crf_eps32.json) is the worst |Q| error of the SAME formula evaluated in NumPy float32 on these
inputs -- the error of the number format, not of the kernel.  Q must lie within 8 * eps32 of the float64 oracle: the factor
covers the kernel's different summation order and the hardware exp.  Labels must equal the oracle's except at pixels whose
float64 top-two margin is under 16 * eps32 (two results 8 * eps32 off the oracle in opposite directions), and such pixels are
at most 1 % of an input.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import sggan_amd
from sggan_amd import _abi as A
from sggan_amd import kernels as K
from sggan_amd import metric as M
from tests import crf_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "city_small")
P = dict(max_iter=O.MAX_ITER, pos_w=O.POS_W, pos_xy_std=O.POS_XY_STD, bi_w=O.Bi_W, bi_xy_std=O.Bi_XY_STD, bi_rgb_std=O.Bi_RGB_STD)
CASES = sorted(O.CASES)
_Q = {}


def _dev(name):
    img, probs = O.case_inputs(name)
    return torch.as_tensor(np.array(img)).cuda(), torch.as_tensor(np.array(probs)).cuda()


def _q(name):
    """The device result of a shared input, computed once per session."""
    if name not in _Q:
        img, probs = _dev(name)
        _Q[name] = K.dense_crf(img, probs=probs, **P).cpu().numpy()
    return _Q[name]


def _labels_agree(q_dev_labels, q64, eps):
    """Compares labels outside the near-tie pixels; returns the share left out."""
    near = O.top2_margin(q64) < 16 * eps
    want = np.argmax(q64, axis=0)
    assert np.array_equal(np.asarray(q_dev_labels)[~near], want[~near])
    return float(near.mean())


@pytest.mark.parametrize("name", CASES)
def test_marginals_within_8_eps32_of_the_oracle(name):
    eps = O.golden_eps32()
    err = float(np.abs(_q(name).astype(np.float64) - O.case_q64(name)).max())
    print(f"{name}: max |Q - oracle| = {err:.3e}, bound 8 * eps32 = {8 * eps:.3e}")
    assert err <= 8 * eps


@pytest.mark.parametrize("name", CASES)
def test_labels_equal_the_oracle_outside_near_ties(name):
    share = _labels_agree(np.argmax(_q(name), axis=0), O.case_q64(name), O.golden_eps32())
    print(f"{name}: near-tie share {share:.4f}")
    assert share <= 0.01


@pytest.mark.parametrize("name", ["tiny34", "ragged34"])
def test_two_launches_give_the_same_bits(name):
    img, probs = _dev(name)
    again = K.dense_crf(img, probs=probs, **P).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), _q(name).view(np.uint32))


@pytest.mark.parametrize("name", ["smooth3", "ragged34"])
def test_no_steps_and_zero_weights_are_softmax_of_the_unary(name):
    """MAX_ITER = 0 returns Q_0 = softmax(-U); with both weights zero every step adds an exact zero, so ten steps return the
    same bits.  Bound of an f32 softmax over C terms against float64: the exp, C additions, one division -- (C + 8) * 2^-24."""
    img, probs = _dev(name)
    C = probs.shape[0]
    q0 = K.dense_crf(img, probs=probs, **{**P, "max_iter": 0}).cpu().numpy()
    want = O.dense_crf_matrix(*O.case_inputs(name), max_iter=0)
    assert np.abs(q0.astype(np.float64) - want).max() <= (C + 8) * 2.0 ** -24
    assert np.abs(q0.sum(axis=0, dtype=np.float64) - 1.0).max() <= (C + 8) * 2.0 ** -24
    qz = K.dense_crf(img, probs=probs, **{**P, "pos_w": 0.0, "bi_w": 0.0}).cpu().numpy()
    assert np.array_equal(qz.view(np.uint32), q0.view(np.uint32))


def test_constant_image_and_unary_stay_uniform():
    img = torch.full((6, 9, 3), 77, dtype=torch.uint8, device="cuda")
    q = K.dense_crf(img, probs=torch.full((4, 6, 9), 0.25, device="cuda"), **P).cpu().numpy()
    assert np.abs(q.astype(np.float64) - 0.25).max() <= 12 * 2.0 ** -24


@pytest.mark.parametrize("name", ["tiny3", "ragged34"])
def test_fused_unary_and_ready_unary_agree_bitwise(name):
    img, probs = _dev(name)
    H, W = img.shape[:2]
    U = torch.as_tensor(O.unary_from_softmax(O.case_inputs(name)[1]).reshape(-1, H, W)).cuda()      # correctly rounded -log(clip(p))
    ready = K.dense_crf(img, unary=U, **P).cpu().numpy()
    assert np.array_equal(ready.view(np.uint32), _q(name).view(np.uint32))


def test_workspace_too_small_is_refused_and_the_queried_size_suffices():
    name = "ragged34"
    img, probs = _dev(name)
    C, H, W = probs.shape
    need = K.dense_crf_workspace_bytes(H, W, C)
    assert need > 0
    guard = 4096
    buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.zeros((C, H, W), dtype=torch.float32, device="cuda")
    args = (K._p(img), K._p(probs), None, H, W, C, O.MAX_ITER, 3.0, 1.0, 4.0, 67.0, 3.0, K._p(out), K._p(buf))
    assert A.lib().sgg_dense_crf(*args, need - 1, K._s()) == A.EWORKSPACE              # status only: nothing was launched
    torch.cuda.synchronize()
    assert not out.any() and bool((buf == 0xA5).all())
    q = K.dense_crf(img, probs=probs, workspace=buf[:need], **P).cpu().numpy()         # exactly the queried size
    assert np.array_equal(q.view(np.uint32), _q(name).view(np.uint32))
    assert bool((buf[need:] == 0xA5).all())                                            # and nothing past it was written


def test_metric_dense_crf_takes_numpy_or_tensors():
    img, probs = O.case_inputs("tiny34")
    q = M.dense_crf(np.array(img), np.array(probs))
    assert isinstance(q, np.ndarray) and q.dtype == np.float32 and np.array_equal(q.view(np.uint32), _q("tiny34").view(np.uint32))
    qt = M.dense_crf(*_dev("tiny34"))
    assert isinstance(qt, torch.Tensor) and qt.is_cuda and np.array_equal(qt.cpu().numpy().view(np.uint32), q.view(np.uint32))
    qu = M.dense_crf(np.array(img), np.array(probs).astype(np.uint8))                  # the score functions pass a uint8 one-hot mask
    assert np.array_equal(qu.view(np.uint32), q.view(np.uint32))
    with pytest.raises(ValueError):
        M.dense_crf(np.array(img).transpose(1, 0, 2), np.array(probs))


# ---- end to end on the fixture folder, 32 x 64 -----------------------------------------------------------------------------
def _args(**kw):
    return sggan_amd.default_args(ngf=8, ndf=8, n_blocks=2, dtype="f32", image_height=32, image_width=64, dataset_dir=FIX, **kw)


@pytest.fixture(scope="module")
def city():
    """(samples with the class mask, the NumPy restatement's labels and marginals on the oracle) of testA at 32 x 64."""
    from sggan_amd import data as D
    from sggan_amd.utils import convert_image_dtype_uint8
    a = _args(crf=True)
    samples = list(D.directory_test_samples(a, D.DatasetCache(FIX, "testA", device="cuda", with_class=True))())
    assert len(samples) == 1 and len(samples[0]) == 4 and samples[0][3].shape == (32, 64, 34)
    name, image, seg, mask = samples[0]
    rescaled = convert_image_dtype_uint8(image[None])
    lt, lp, q = O.scores_mask_sample_crf_numpy(mask[None], rescaled, O.dense_crf_matrix)
    return {"samples": samples, "mask": mask[None], "rescaled": rescaled, "lt": lt, "lp": lp, "q": q}


def test_class_mask_is_optional_and_one_hot(city):
    from sggan_amd import data as D
    plain = list(D.directory_test_samples(_args(), D.DatasetCache(FIX, "testA", device="cuda", with_class=False))())
    assert len(plain[0]) == 3 and plain[0][0] == city["samples"][0][0]
    assert all(np.array_equal(a, b) for a, b in zip(plain[0][1:], city["samples"][0][1:3]))
    mask = city["mask"]
    assert mask.dtype == np.float32 and set(np.unique(mask).tolist()) == {0.0, 1.0} and np.array_equal(mask.sum(axis=-1), np.ones((1, 32, 64)))
    assert len(np.unique(mask.argmax(axis=-1))) > 3


def test_crf_score_functions_match_the_numpy_restatement(city):
    eps = O.golden_eps32()
    lt, lp = M.scores_mask_sample_crf(city["mask"], city["rescaled"])
    assert lt.shape == (1, 64, 32) and lp.shape == (1, 64, 32) and np.array_equal(lt, city["lt"])
    share = _labels_agree(lp[0], city["q"], eps)
    print(f"city 32x64: near-tie share {share:.4f}")
    assert share <= 0.01
    fake = np.random.default_rng(5).integers(0, 256, (1, 32, 64, 3)).astype(np.uint8)
    lt2, lp2 = M.scores_fake_mask_crf(city["mask"], city["rescaled"], fake)
    assert np.array_equal(lt2, np.argmax(fake.transpose(0, 3, 2, 1), axis=1)) and np.array_equal(lp2, lp)
    ltf, _ = M.scores_fake_mask_crf(city["mask"], city["rescaled"], (fake / 255.0).astype(np.float32))     # a float image is converted
    assert ltf.shape == (1, 64, 32) and ltf.max() <= 2
    s = M.scores(lt, lp, n_class=34)
    assert 0.0 <= s["Mean IoU"] <= 1.0 and s["Overall Acc"] > 0.5            # the CRF of a one-hot mask keeps most of its labels


REF_TAGS = ["Overall Accuracy", "Mean Accuracy", "Frequency Weighted Accuracy", "Mean IoU"]


def test_test_during_train_writes_the_crf_scalars_after_the_reference_ones(city):
    from sggan_amd.utils import SummarySink
    a = _args(crf=True, test_dir=None)
    sink = SummarySink()
    _, score = sggan_amd.sggan(a).test_during_train(3, a, city["samples"], sink)
    assert [r["tag"] for r in sink.records] == REF_TAGS + ["CRF " + t for t in REF_TAGS] and all(r["step"] == 3 for r in sink.records)
    want = M.scores(*M.scores_mask_sample_crf(city["mask"], city["rescaled"]), n_class=34)
    got = {r["tag"]: r["value"] for r in sink.records}
    assert got["CRF Overall Accuracy"] == want["Overall Acc"] and got["CRF Mean IoU"] == want["Mean IoU"]
    assert score["CRF"]["Mean Acc"] == want["Mean Acc"]
    with pytest.raises(ValueError):                                                      # --crf without the class mask is an error
        sggan_amd.sggan(a).test_during_train(3, a, [s[:3] for s in city["samples"]], SummarySink())


def test_crf_off_leaves_the_sink_as_a_model_without_the_flag(city):
    from sggan_amd.utils import SummarySink
    off, bare = _args(crf=False, test_dir=None), _args(test_dir=None)
    del bare.crf                                                                          # a namespace from before the flag existed
    records = []
    for a in (off, bare):
        sink = SummarySink()
        sggan_amd.sggan(a).test_during_train(1, a, [s[:3] for s in city["samples"]], sink)
        records.append(sink.records)
    assert records[0] == records[1] and [r["tag"] for r in records[0]] == REF_TAGS


def test_get_labels_matches_the_reference_transposes():
    m = sggan_amd.sggan(_args())
    rng = np.random.default_rng(2)
    label, pred = rng.random((1, 6, 9, 3)).astype(np.float32), rng.random((1, 6, 9, 3)).astype(np.float32)
    for wrap in (lambda x: x, torch.as_tensor):
        lt, lp = m.get_labels(wrap(label), wrap(pred))
        assert np.array_equal(lt, label.transpose(0, 3, 2, 1)) and np.array_equal(lp, pred.transpose(0, 3, 2, 1))
    sq_label, sq_pred = rng.random((1, 8, 8, 3)).astype(np.float32), rng.random((1, 8, 8, 3)).astype(np.float32)
    lt, lp = m.get_labels(sq_label, torch.as_tensor(sq_pred), crf=True)                   # crf_wrapper, model.py:282-296
    image = (sq_label * 255).astype(np.uint8)
    assert np.array_equal(lt, image) and lp.shape == (1, 3, 8, 8)
    assert np.array_equal(lp[0], M.dense_crf(image[0], sq_pred.transpose(0, 3, 2, 1)[0]))
