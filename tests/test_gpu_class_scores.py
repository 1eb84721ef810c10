"""Class-level evaluation on the GPU (csrc/evalseg.hip) against the NumPy restatement of tests/class_scores_oracle.py.

Labels, confusion matrices and the boundary band are integer: EQUAL to the oracle.  Probabilities: atol 1e-5 against the
float64 oracle -- a term with e > 1e-7 has an exponent argument below 16, so the f32 rounding of the argument (16 * 2^-24 ~ 1e-6)
plus <= 2 ulp of expf stays under 2e-6 relative, and the sum has <= 64 terms; a row sums to 1 within 1e-6.
"""
import os

import numpy as np
import pytest
import torch

import sggan_amd
from sggan_amd import kernels as K
from sggan_amd import metric as M
from sggan_amd import segment_class as SC
from tests import class_scores_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 5, 7), (1, 16, 33), (3, 17, 259)]          # one pixel; vector tails; a batch stride; more than one block
KINDS = ["f32c8", "bf16c8", "f32c3", "u8c3", "u8c4", "u8c3_unaligned"]
SPECIAL = np.array([-1.0, 1.0, -1.0001, 1.0001, np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0, -3.0, 0.99999994], dtype=np.float32)


def _palette(name):
    if name == "k1":
        return np.array([0x102030], dtype=np.uint32), np.array([3], dtype=np.uint8)
    if name == "k19":
        return O.city_palette()
    return O.random_palette(64, 34, seed=64)


def _tie_colour(keys):
    """A colour whose two nearest palette entries are equally far (the midpoint of two entries with even channel sums), or None."""
    rgb = O.key_rgb(keys)
    for i in range(len(rgb)):
        for j in range(i + 1, len(rgb)):
            if ((rgb[i] + rgb[j]) % 2 == 0).all():
                mid = (rgb[i] + rgb[j]) // 2
                d = np.sort(O.distances(mid, keys))
                if d[0] == d[1]:
                    return mid
    return None


def _colours(shape, keys, seed):
    """int (N,H,W,3) 8-bit colours and the flat indices of the constructed ones: random colours, then -- as far as the pixels go
    -- entry 0 exactly, colours at squared distance 9 and 10 from it, a colour equidistant from its two nearest entries, and
    every other palette colour exactly."""
    rng = np.random.default_rng(seed)
    N, H, W = shape
    q = rng.integers(0, 256, (N * H * W, 3))
    rgb = O.key_rgb(keys)
    special = [rgb[0], np.clip(rgb[0] + (3, 0, 0), 0, 255), np.clip(rgb[0] + (3, 1, 0), 0, 255)]           # d2 = 0, 9, 10 from entry 0
    tie = _tie_colour(keys)
    if tie is not None:
        special.append(tie)
    special += list(rgb[1:])
    special = np.array(special[:max(1, len(q) - len(q) // 3)])
    where = rng.permutation(len(q))[:len(special)]
    q[where] = special
    return q.reshape(N, H, W, 3), where


def _input_np(kind, shape, keys, seed):
    """The input of one case as a NumPy array (float kinds: float32, before any bf16 rounding): the colours of _colours in the
    input kind; float kinds also hold -1, 1, values just outside [-1,1], NaN and infinities in pixels _colours did not construct."""
    q, where = _colours(shape, keys, seed)
    N, H, W = shape
    rng = np.random.default_rng(seed + 1)
    if kind.startswith("u8"):
        C = 4 if kind == "u8c4" else 3
        img = rng.integers(0, 256, (N, H, W, C)).astype(np.uint8)
        img[..., :3] = q
        return img
    C = 3 if kind == "f32c3" else 8
    x = rng.uniform(-1, 1, (N, H, W, C)).astype(np.float32)
    x[..., :3] = ((q + 0.5) / 127.5 - 1.0).astype(np.float32)            # the middle of colour q's interval: survives bf16 rounding
    flat = x.reshape(-1, C)
    free = np.setdiff1d(np.arange(len(flat)), where)
    rows = rng.permutation(free)[:len(SPECIAL)]
    flat[rows, rng.integers(0, 3, len(rows))] = SPECIAL[:len(rows)]
    return x


def _input(kind, shape, keys, seed):
    """(device tensor, the array the oracle decodes)."""
    img = _input_np(kind, shape, keys, seed)
    if kind == "u8c3_unaligned":
        buf = torch.zeros(img.size + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.as_tensor(img).cuda().view(-1)
        t = buf[1:].view(img.shape)
        assert t.data_ptr() % 4 == 1
        return t, img
    t = torch.as_tensor(img).cuda()
    if kind == "bf16c8":
        t = t.to(torch.bfloat16)
        return t, t.float().cpu().numpy()
    return t, img


@pytest.mark.parametrize("pal", ["k1", "k19", "k64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_labels_equal_the_oracle(kind, shape, pal):
    keys, classes = _palette(pal)
    t, ref = _input(kind, shape, keys, seed=sum(shape) + len(keys))
    for other, md in ((0, -1), (33, 9), (0, 0)):
        got = M.palette_labels(t, (keys, classes), other_class=other, max_dist2=md)
        assert got.dtype == torch.int32 and tuple(got.shape) == shape
        want = O.labels(ref, keys, classes, other, md)
        assert np.array_equal(got.cpu().numpy(), want), (kind, shape, pal, other, md)
    if pal != "k1" and np.prod(shape) > 8:                               # the constructed cases are in the input
        d = O.distances(O.colours(ref), keys)
        s = np.sort(d, axis=-1)
        assert (s[..., 0] == s[..., 1]).any() and (d.min(axis=-1) == 0).any()
    if pal == "k1" and np.prod(shape) > 8:
        d = O.distances(O.colours(ref), keys)[..., 0]
        assert (d == 9).any() and (d == 10).any()


def test_builtin_palette_is_the_default_and_numpy_input_works():
    keys, classes = SC.palette()
    t, ref = _input("u8c3", (2, 5, 7), keys, seed=3)
    assert np.array_equal(M.palette_labels(t).cpu().numpy(), O.labels(ref, keys, classes))
    assert np.array_equal(M.palette_labels(ref).cpu().numpy(), O.labels(ref, keys, classes))
    assert np.array_equal(M.palette_labels(ref[0]).cpu().numpy(), O.labels(ref[:1], keys, classes))            # (H,W,C) -> one image


# ---- fused scoring ---------------------------------------------------------------------------------------------------------
def _score_case(n_class, kind, shape, seed):
    keys, classes = O.random_palette(min(64, 3 * n_class), n_class, seed)
    t, ref = _input(kind, shape, keys, seed)
    rng = np.random.default_rng(seed + 7)
    truth = rng.integers(0, min(n_class + 3, 256), shape).astype(np.uint8)                # some >= n_class: ignored
    truth.reshape(-1)[::5] = classes[rng.integers(0, len(classes), truth.reshape(-1)[::5].size)]
    truth.reshape(-1)[1:3] = (n_class, n_class + 2)
    select = (rng.integers(0, 3, shape) * 7).astype(np.uint8)                            # 0, 7 or 14: non-zero counts
    return (keys, classes), t, ref, truth, select


@pytest.mark.parametrize("kind", ["bf16c8", "f32c3", "u8c3", "u8c4", "u8c3_unaligned"])
@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 17, 259)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("n_class", [8, 34, 64])
def test_hist_equals_the_oracle(n_class, shape, kind):
    pal, t, ref, truth, select = _score_case(n_class, kind, shape, seed=n_class + shape[2])
    tt, ts = torch.as_tensor(truth).cuda(), torch.as_tensor(select).cuda()
    pred = O.labels(ref, *pal)
    assert (truth >= n_class).any() and (truth < n_class).any()
    h = M.scores_class_fake(tt, t, n_class, pal)
    assert h.dtype == torch.int64 and tuple(h.shape) == (n_class, n_class) and h.is_cuda
    assert np.array_equal(h.cpu().numpy(), O.hist(truth, pred, n_class))
    # the fused launch equals decode followed by the confusion-matrix kernel
    assert np.array_equal(h.cpu().numpy(), M._fast_hist(tt, M.palette_labels(t, pal), n_class))
    # select
    hs = torch.zeros_like(h)
    K.palette_decode(t, pal, truth=tt, select=ts, n_class=n_class, hist=hs, want_labels=False)
    assert np.array_equal(hs.cpu().numpy(), O.hist(truth, pred, n_class, select))
    # two calls into one hist add up; a second run gives the same bits; labels and hist from ONE launch agree with both
    lab, h2 = K.palette_decode(t, pal, truth=tt, n_class=n_class, hist=h.clone())
    assert np.array_equal(h2.cpu().numpy(), 2 * O.hist(truth, pred, n_class)) and np.array_equal(lab.cpu().numpy(), pred)
    assert torch.equal(M.scores_class_fake(tt, t, n_class, pal), h)
    # predictions >= n_class (other_class past the score's classes) are ignored
    far = O.labels(ref, *pal, other_class=200, max_dist2=2000)
    assert (far == 200).any() and (far != 200).any()
    hf = M.scores_class_fake(tt, t, n_class, pal, other_class=200, max_dist2=2000)
    assert np.array_equal(hf.cpu().numpy(), O.hist(truth, far, n_class))


def test_scores_from_hist_equals_scores_of_the_label_lists():
    pal, t, ref, truth, _ = _score_case(34, "bf16c8", (3, 17, 259), seed=5)
    pred = O.labels(ref, *pal)
    h = M.scores_class_fake(torch.as_tensor(truth).cuda(), t, 34, pal)
    np.testing.assert_equal(M.scores_from_hist(h), M.scores(list(truth.astype(np.int32)), list(pred), n_class=34))
    np.testing.assert_equal(M.scores_from_hist(h.cpu().numpy().ravel()), M.scores_from_hist(h))


# ---- boundary band ---------------------------------------------------------------------------------------------------------
def _maps(N, H, W, seed):
    """Block-constant class maps with boundaries on tile edges (x = 64 k, y = 16 k), single pixels on the image border and some
    speckle; image 0 is constant, so anything set there leaked from another image."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = ((x // 64 + 2 * (y // 16)) % 5).astype(np.uint8)
    cls = np.stack([base.copy() for _ in range(N)])
    for n in range(N):
        cls[n, 0, 0] = 9; cls[n, H - 1, W - 1] = 9; cls[n, H // 2, 0] = 8; cls[n, 0, W // 2] = 8
        idx = rng.integers(0, H * W, max(1, H * W // 97))
        cls[n].reshape(-1)[idx] = rng.integers(0, 34, len(idx))
    if N > 1:
        cls[0] = 6
    return cls


@pytest.mark.parametrize("r", [0, 1, 3, 8])
@pytest.mark.parametrize("shape", [(1, 2, 3), (2, 16, 65), (2, 33, 257), (1, 1, 1), (3, 17, 64)], ids=lambda s: "x".join(map(str, s)))
def test_band_equals_the_oracle(shape, r):
    cls = _maps(*shape, seed=r + shape[2])
    got = K.class_boundary_band(torch.as_tensor(cls).cuda(), r).cpu().numpy()
    want = O.band(cls, r)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    if r == 0 or shape[0] > 1:
        assert not got[0].any()                                           # r = 0: all zeros; a constant image: no leak across images
    if r > 0 and shape[1] * shape[2] > 1:
        assert got[-1].any() and set(np.unique(got).tolist()) <= {0, 1}


def test_band_scores_count_only_the_band():
    pal, t, ref, truth, _ = _score_case(34, "bf16c8", (2, 16, 65), seed=11)
    truth = _maps(2, 16, 65, seed=2)
    h = M.scores_class_fake(truth, t, 34, pal, band_radius=3)
    assert np.array_equal(h.cpu().numpy(), O.hist(truth, O.labels(ref, *pal), 34, O.band(truth, 3)))
    assert 0 < int(h.sum()) < truth.size


# ---- probabilities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32c8", "bf16c8", "f32c3", "u8c3"])
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 16, 33)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", ["k19", "k19_other", "k64", "k1"])
def test_probabilities_within_1e5_of_the_oracle(case, shape, kind):
    pal = _palette(case.split("_")[0])
    n_class = {"k19": 34, "k64": 64, "k1": 8}[case.split("_")[0]]
    kw = dict(sigma=32.0, other_class=0, max_dist2=400) if case == "k19_other" else dict(sigma=8.0 if case == "k64" else 32.0)
    t, ref = _input(kind, shape, pal[0], seed=len(case) + shape[2])
    got = M.palette_probs(t, n_class, pal, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0], n_class, shape[1], shape[2])
    got = got.cpu().numpy()
    want = O.probs(ref, *pal, n_class, **kw)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{case} {kind} {shape}: max |p - oracle| = {err:.3e}")
    assert err <= 1e-5
    assert np.abs(got.sum(axis=1, dtype=np.float64) - 1.0).max() <= 1e-6
    m = O.class_distances(ref, *pal, n_class, kw.get("other_class", 0), kw.get("max_dist2", -1))
    absent = np.moveaxis(m == O.NONE, -1, 1)
    assert absent.any() and np.array_equal(got[absent], np.zeros(int(absent.sum()), dtype=np.float32))          # exactly 0
    if case == "k19_other":
        assert not absent[:, 0].any() and (got[:, 0] > 0).all()           # class 0 has no colour: it lives on the pseudo-distance
    s = np.sort(m, axis=-1)
    clear = (s[..., 0] != s[..., 1]) if n_class > 1 else np.ones(shape, dtype=bool)
    lab = M.palette_labels(t, pal, other_class=kw.get("other_class", 0), max_dist2=kw.get("max_dist2", -1)).cpu().numpy()
    assert clear.any() and np.array_equal(np.argmax(got, axis=1)[clear], lab[clear])


# ---- CRF composition -------------------------------------------------------------------------------------------------------
def test_scores_class_fake_crf_is_the_composition_of_the_public_pieces():
    rng = np.random.default_rng(8)
    pal = O.random_palette(12, 8, seed=12)
    t, ref = _input("f32c3", (2, 16, 16), pal[0], seed=4)
    truth = rng.integers(0, 8, (2, 16, 16)).astype(np.uint8)
    photo = rng.integers(0, 256, (2, 16, 16, 3)).astype(np.float32)
    h = M.scores_class_fake_crf(truth, photo, t, 8, pal)
    want = np.zeros((8, 8), dtype=np.int64)
    probs = M.palette_probs(t, 8, pal)
    for n in range(2):
        q = M.dense_crf(torch.as_tensor(photo[n].astype(np.uint8)).cuda(), probs[n])
        want += M._fast_hist(truth[n], torch.argmax(q, dim=0), 8)
    assert h.dtype == torch.int64 and np.array_equal(h.cpu().numpy(), want) and int(want.sum()) == 2 * 16 * 16


# ---- the PNG save_images writes --------------------------------------------------------------------------------------------
def test_decoding_the_saved_png_equals_decoding_the_tensor(tmp_path):
    from PIL import Image
    from sggan_amd.utils import save_images
    pal = O.city_palette()
    rng = np.random.default_rng(21)
    fake = rng.uniform(-1, 1, (1, 17, 33, 3)).astype(np.float32)
    fake.reshape(-1)[:6] = [-1, 1, -1, 1, 0, 0.99999994]
    t = torch.as_tensor(fake).cuda()
    path = str(tmp_path / "fake.png")
    save_images(t, [1, 1], path)
    png = np.asarray(Image.open(path), dtype=np.uint8)
    assert png.shape == (17, 33, 3)
    from_png, from_tensor = M.palette_labels(png, pal), M.palette_labels(t, pal)
    assert torch.equal(from_png, from_tensor) and np.array_equal(from_tensor.cpu().numpy(), O.labels(fake, *pal))


# ---- learn_palette on the device cache, and the test pass --------------------------------------------------------------------
REF_TAGS = ["Overall Accuracy", "Mean Accuracy", "Frequency Weighted Accuracy", "Mean IoU"]
CLASS_TAGS = ["Class " + t for t in REF_TAGS]


def _args(**kw):
    return sggan_amd.default_args(ngf=8, ndf=8, n_blocks=2, dtype="f32", image_height=32, image_width=32, dataset_dir=O.FIX, test_dir=None, **kw)


@pytest.fixture(scope="module")
def city():
    from sggan_amd import data as D
    cache = D.DatasetCache(O.FIX, "testA", device="cuda", with_class=True)
    pal = SC.learn_palette(cache)
    samples = list(D.directory_test_samples(_args(), cache)())
    assert len(samples) == 1 and samples[0][3].shape == (32, 32, 34)
    return {"cache": cache, "palette": pal, "samples": samples}


def test_learn_palette_on_the_device_cache_equals_the_oracle(city):
    from sggan_amd import data as D
    want = O.learn_palette(O.city_pairs()[2:])                            # the testA pair
    assert all(np.array_equal(a, b) for a, b in zip(city["palette"], want))
    train = SC.learn_palette(D.DatasetCache(O.FIX, "trainA", device="cuda", with_class=True))
    assert all(np.array_equal(a, b) for a, b in zip(train, O.learn_palette(O.city_pairs()[:2])))
    with pytest.raises(ValueError):
        SC.learn_palette(D.DatasetCache(O.FIX, "testA", device="cuda", with_class=False))


def _run(city, **kw):
    from sggan_amd.utils import SummarySink
    a = _args(**kw)
    if kw.get("class_scores"):
        a.class_palette = city["palette"]
    sink = SummarySink()
    fakes, score = sggan_amd.sggan(a).test_during_train(2, a, city["samples"], sink)
    return sink.records, fakes, score


def test_test_during_train_adds_the_class_scalars_after_the_existing_ones(city):
    base, _, base_score = _run(city)
    assert [r["tag"] for r in base] == REF_TAGS
    rec, fakes, score = _run(city, class_scores=True)
    assert rec[:4] == base                                               # the existing scalars: same values, same order
    assert [r["tag"] for r in rec[4:]] == CLASS_TAGS + ["Boundary Class Mean IoU"] and all(r["step"] == 2 for r in rec)
    truth = city["samples"][0][3].argmax(axis=-1)[None]
    pred = O.labels(fakes, *city["palette"])                              # the uint8 fakes the pass returns: the same colours
    want = M.scores_from_hist(O.hist(truth, pred, 34))
    np.testing.assert_equal(score["Class"], want)
    assert set(want) == {"Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU", "Class IoU"}
    got = {r["tag"]: r["value"] for r in rec}
    assert got["Class Overall Accuracy"] == want["Overall Acc"] and got["Class Mean IoU"] == want["Mean IoU"]
    np.testing.assert_equal(score["Class Boundary"], M.scores_from_hist(O.hist(truth, pred, 34, O.band(truth.astype(np.uint8), 3))))
    assert got["Boundary Class Mean IoU"] == score["Class Boundary"]["Mean IoU"]
    np.testing.assert_equal({k: v for k, v in score.items() if k not in ("Class", "Class Boundary", "Class CRF")}, base_score)
    rec0, _, score0 = _run(city, class_scores=True, boundary_px=0)
    assert [r["tag"] for r in rec0] == REF_TAGS + CLASS_TAGS and "Class Boundary" not in score0
    # the threshold: a pixel farther than class_max_dist from every palette colour counts as class 0
    _, _, near = _run(city, class_scores=True, class_max_dist=20)
    np.testing.assert_equal(near["Class"], M.scores_from_hist(O.hist(truth, O.labels(fakes, *city["palette"], 0, 400), 34)))
    with pytest.raises(ValueError):                                       # class_scores without the class mask is an error
        a = _args(class_scores=True)
        sggan_amd.sggan(a).test_during_train(2, a, [s[:3] for s in city["samples"]], None)


def test_without_the_flag_the_sink_is_as_before(city):
    off, _, _ = _run(city, class_scores=False)
    bare, _, _ = _run(city)
    assert off == bare and [r["tag"] for r in bare] == REF_TAGS


def test_with_crf_the_class_crf_scalars_come_last(city):
    from sggan_amd.utils import convert_image_dtype_uint8
    rec, fakes, score = _run(city, crf=True, class_scores=True)
    assert [r["tag"] for r in rec] == REF_TAGS + ["CRF " + t for t in REF_TAGS] + CLASS_TAGS + ["Boundary Class Mean IoU"] + \
        ["Class CRF " + t for t in REF_TAGS]
    truth = city["samples"][0][3].argmax(axis=-1)[None].astype(np.uint8)
    rescaled = convert_image_dtype_uint8(city["samples"][0][1][None])
    want = M.scores_from_hist(M.scores_class_fake_crf(truth, rescaled, fakes, 34, city["palette"]))
    np.testing.assert_equal(score["Class CRF"], want)
    assert rec[-1]["value"] == want["Mean IoU"]


def test_phase_test_logs_the_class_scores_when_the_samples_carry_a_mask(city, tmp_path):
    a = _args(class_scores=True, checkpoint_dir=str(tmp_path / "ckpt"))
    a.test_dir, a.class_palette = str(tmp_path / "out"), city["palette"]
    lines = []
    sggan_amd.sggan(a).test(a, city["samples"], log=lines.append)
    assert sum("Class Mean IoU" in l for l in lines) == 1
    plain = []
    b = _args(checkpoint_dir=str(tmp_path / "ckpt"))
    b.test_dir = str(tmp_path / "out")
    sggan_amd.sggan(b).test(b, city["samples"], log=plain.append)
    assert plain == [l for l in lines if "Class Mean IoU" not in l]
