"""Paired image-quality sums on the GPU (csrc/imgqual.hip) against the float64 NumPy statement of tests/image_quality_oracle.py.

The two integer sums (sum |a-b|, sum (a-b)^2) must EQUAL the oracle.  The SSIM sum, divided by its count, must be within 1e-9
absolute: double rounding over 121 taps is ~1e-14 relative, the cancellation in E[xx] - ux^2 leaves <= ~1e-10 absolute on a
variance that is compared with C2 ~ 58.5, so 1e-9 on a value in [-1, 1] leaves more than two orders of margin -- and a
reordered f32 implementation would not meet it.  Shapes are the smallest that put the valid extent on, one short of and one
past the tile edges.
"""
import os

import numpy as np
import pytest
import torch

import sggan_amd
from sggan_amd import _abi as A
from sggan_amd import kernels as K
from sggan_amd import metric as M
from tests import image_quality_oracle as O

pytestmark = pytest.mark.gpu

IQ_TH, IQ_TW = 16, 32                                    # csrc/imgqual.hip (tests/test_image_quality_cpu.py reads both)
SSIM_ATOL = 1e-9


def _u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def _dev(x):
    return torch.as_tensor(x).cuda()


def _bits(t):
    return t.view(torch.int64).cpu().numpy()


def _check(got, a_ref, b_ref, what=""):
    """got (N,3) device rows against the oracle on the arrays the operands hold; returns the rows as NumPy."""
    g = got.cpu().numpy()
    want = O.sums(a_ref, b_ref)
    H, W = np.asarray(a_ref).shape[-3:-1]
    count = O.counts(H, W)[1]
    err = float(np.abs(g[:, 2] / count - want[:, 2] / count).max())
    print(f"{what} {H}x{W}: sad {g[:, 0].tolist()} ssd {g[:, 1].tolist()} ssim {(g[:, 2] / count).tolist()} |ssim - oracle| {err:.3e}")
    assert got.dtype == torch.float64 and g.shape == want.shape
    assert np.array_equal(g[:, :2], want[:, :2]), (what, g[:, :2], want[:, :2])
    assert err <= SSIM_ATOL, (what, err)
    return g


# ---- valid extents at the tile edges -----------------------------------------------------------------------------------------
EXTENTS = sorted({(vh, vw) for vh in (1, IQ_TH - 1, IQ_TH, IQ_TH + 1) for vw in (1, IQ_TW - 1, IQ_TW, IQ_TW + 1, 2 * IQ_TW + 3)}
                 | {(1, 1), (1, IQ_TW + 1), (IQ_TH + 1, 1)})         # 11 x 11; 11 x (IQ_TW + 11); (IQ_TH + 11) x 11


@pytest.mark.parametrize("vh,vw", EXTENTS, ids=lambda v: str(v))
def test_sums_at_the_tile_edges(vh, vw):
    H, W = vh + 10, vw + 10
    a, b = _u8((1, H, W, 3), 100 * vh + vw), _u8((1, H, W, 3), 100 * vh + vw + 1)
    g = _check(K.image_quality(_dev(a), _dev(b)), a, b, "edges")
    assert g[0, 0] > 0 and 0 < abs(g[0, 2]) < 3 * vh * vw


# ---- image indexing ----------------------------------------------------------------------------------------------------------
def test_each_image_of_a_batch_equals_its_own_call_bit_for_bit():
    H, W = IQ_TH + 13, IQ_TW + 15                          # 2 x 2 tiles per image
    a, b = _u8((3, H, W, 3), 7), _u8((3, H, W, 3), 8)
    b[1] = np.clip(a[1].astype(np.int64) + 3, 0, 255)     # three different pairs: far, near, and ...
    b[2, :, : W // 2] = a[2, :, : W // 2]                  # ... half identical
    got = K.image_quality(_dev(a), _dev(b))
    g = _check(got, a, b, "batch")
    assert len({tuple(r) for r in g.tolist()}) == 3
    for n in range(3):
        one = K.image_quality(_dev(a[n:n + 1]), _dev(b[n:n + 1]))
        assert np.array_equal(_bits(one)[0], _bits(got)[n]), n


# ---- every operand form ------------------------------------------------------------------------------------------------------
def _float_image(shape, seed, bf16):
    """float32 (N,H,W,3) in the middle of the colours' intervals (they survive bf16 rounding), with -1, 1, values outside
    [-1,1], a NaN and the two sides of a quantisation step (of the f32 grid, or of the bf16 grid) written over some pixels."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, shape)
    x = ((q + 0.5) / 127.5 - 1.0).astype(np.float32)
    if bf16:
        grid = torch.arange(0x3E80, 0x3F00, dtype=torch.int16).view(torch.bfloat16).float().numpy()       # the bf16 values of [0.25, 0.5)
        qs = O.quantise(grid.reshape(1, 1, -1, 1).repeat(3, axis=3))[0, 0, :, 0]
        k = int(np.nonzero(np.diff(qs))[0][0])
        step = [grid[k], grid[k + 1]]
    else:
        edge = np.float32(2.0 * 100 / 255 - 1.0)
        step = [np.nextafter(edge, np.float32(-2)), edge, np.nextafter(edge, np.float32(2))]
    sq = O.quantise(np.array(step, dtype=np.float32).reshape(1, 1, -1, 1).repeat(3, axis=3))[0, 0, :, 0]
    assert len(set(sq.tolist())) == 2, sq                  # the step lies between them
    special = np.array([-1.0, 1.0, -1.0001, 1.0001, -1.5, 3.0, np.nan, np.inf, -np.inf, 0.99999994] + step, dtype=np.float32)
    flat = x.reshape(-1)
    where = rng.permutation(flat.size)[:len(special)]
    flat[where] = special
    return x


def _forms(x, bf16):
    """{form: (device tensor, the float / uint8 array it holds)} of one image in every layout of its type."""
    N, H, W, _ = x.shape
    dtype = torch.bfloat16 if bf16 else torch.float32
    t3 = _dev(x).to(dtype).contiguous()
    held = t3.float().cpu().numpy()
    quant = O.quantise(held).astype(np.uint8)
    pad = torch.full((N, H, W, A.CPAD), 0.25, dtype=dtype, device="cuda")
    pad[..., :3] = t3
    out = {"c3": (t3, held), "cpad": (pad.contiguous(), held)}
    assert out["cpad"][0].data_ptr() % 16 == 0
    for name, shift in (("cpad_off_pixel", A.CPAD), ("cpad_off_element", 1)):          # one pixel on: still 16-byte aligned; one
        buf = torch.zeros(pad.numel() + shift, dtype=dtype, device="cuda")             # element on: unaligned -> the scalar path
        buf[shift:] = pad.reshape(-1)
        view = buf[shift:].view(pad.shape)
        assert (view.data_ptr() % 16 == 0) == (name == "cpad_off_pixel")
        out[name] = (view, held)
    u4 = np.concatenate([quant, _u8((N, H, W, 1), 5)], axis=3)
    out["u8c3"], out["u8c4"] = (_dev(quant), quant), (_dev(u4), u4)
    return out


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_every_operand_form_gives_the_same_bits(bf16):
    shape = (2, 19, IQ_TW + 13, 3)
    forms = _forms(_float_image(shape, 11 + bf16, bf16), bf16)
    other = _u8(shape, 13)
    rows = {}
    for name, (t, held) in forms.items():
        rows[name] = _bits(K.image_quality(t, _dev(other)))
        _check(K.image_quality(t, _dev(other)), held, other, name)
        assert np.array_equal(_bits(K.image_quality(_dev(other), t)), rows[name]), name          # as the second operand
    for name in forms:
        assert np.array_equal(rows[name], rows["c3"]), name
    # float against float, one of each layout
    pair = K.image_quality(forms["cpad"][0], forms["cpad_off_element"][0])
    assert np.array_equal(pair.cpu().numpy(), np.array([[0.0, 0.0, O.counts(*shape[1:3])[1]]] * 2))


# ---- exactness ---------------------------------------------------------------------------------------------------------------
def test_identical_operands_give_zero_sums_and_the_count_exactly_and_the_operands_commute():
    H, W = IQ_TH + 12, IQ_TW + 12
    count = float(O.counts(H, W)[1])
    a = _u8((2, H, W, 3), 21)
    same = K.image_quality(_dev(a), _dev(a.copy())).cpu().numpy()
    assert np.array_equal(same, np.array([[0.0, 0.0, count]] * 2))
    x = _dev(_float_image((2, H, W, 3), 22, True)).to(torch.bfloat16)
    own = _dev(O.quantise(x.float().cpu().numpy()).astype(np.uint8))                  # bf16 against its own quantised uint8
    assert np.array_equal(K.image_quality(x, own).cpu().numpy(), np.array([[0.0, 0.0, count]] * 2))
    b = _u8((2, H, W, 3), 23)
    ab, ba = K.image_quality(_dev(a), _dev(b)), K.image_quality(_dev(b), _dev(a))
    assert np.array_equal(_bits(ab), _bits(ba)) and ab[0, 0].item() > 0
    xa, xb = K.image_quality(x, _dev(b)), K.image_quality(_dev(b), x)
    assert np.array_equal(_bits(xa), _bits(xb))


def test_two_calls_give_the_same_bits_whatever_the_workspace_held():
    H, W = 2 * IQ_TH + 11, 2 * IQ_TW + 13
    a, b = _dev(_u8((2, H, W, 3), 31)), _dev(_u8((2, H, W, 3), 32))
    need = K.image_quality_workspace_bytes(2, H, W)
    assert need == 2 * 24 * 3 * 3
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    first = K.image_quality(a, b, workspace=ws).clone()
    ws.fill_(0xFF)                                         # NaN bytes
    out = torch.full((2, 3), float("nan"), dtype=torch.float64, device="cuda")
    second = K.image_quality(a, b, out=out, workspace=ws)
    assert second is out and np.array_equal(_bits(first), _bits(second))
    _check(second, a.cpu().numpy(), b.cpu().numpy(), "poisoned workspace")
    with pytest.raises(A.SggError, match="SGG_EWORKSPACE"):
        K.image_quality(a, b, workspace=ws[:need - 8])
    with pytest.raises(A.SggError, match="SGG_EUNSUPPORTED"):
        K.image_quality(a[:, :10], b[:, :10])


# ---- piecewise-constant label-like images: the cancellation case -----------------------------------------------------------------
def test_piecewise_constant_images_with_a_one_pixel_shift():
    H, W = 2 * IQ_TH + 9, 2 * IQ_TW + 12
    palette = np.array([[128, 64, 128], [70, 70, 70], [0, 0, 0], [255, 255, 255], [220, 20, 60], [0, 0, 142]], dtype=np.uint8)
    rng = np.random.default_rng(41)
    idx = rng.integers(0, len(palette), (2, (H + 1) // 7 + 1, (W + 1) // 9 + 1)).repeat(7, axis=1).repeat(9, axis=2)
    a = palette[idx[:, :H, :W]]
    b = palette[idx[:, 1:H + 1, 1:W + 1]]                                               # the same map one pixel up and left
    assert a.shape == (2, H, W, 3) and not np.array_equal(a, b) and (a == b).mean() > 0.5
    g = _check(K.image_quality(_dev(a), _dev(b)), a, b, "label maps")
    flat = (O.ssim_map(O.quantise(a), O.quantise(a)) == 1.0).all()                     # (constant windows are exactly 1 in the oracle)
    assert flat and 0 < g[0, 2] < O.counts(H, W)[1]
    af = _dev(((a.astype(np.float32) + 0.5) / 127.5 - 1.0)).to(torch.bfloat16)          # the generator's side as bf16
    assert np.array_equal(_bits(K.image_quality(af, _dev(b))), _bits(K.image_quality(_dev(a), _dev(b))))


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_call_replays_from_a_captured_graph_with_rewritten_inputs():
    H, W = IQ_TH + 14, IQ_TW + 17
    imgs = [(_u8((2, H, W, 3), 50 + k), _float_image((2, H, W, 3), 60 + k, True)) for k in range(3)]
    a = _dev(imgs[0][0])
    b = torch.zeros((2, H, W, A.CPAD), dtype=torch.bfloat16, device="cuda")
    b[..., :3] = _dev(imgs[0][1]).to(torch.bfloat16)
    ws = torch.empty(K.image_quality_workspace_bytes(2, H, W), dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    K.image_quality(a, b, out=out, workspace=ws)
    torch.cuda.synchronize()
    warm = out.clone()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.image_quality(a, b, out=out, workspace=ws)
    torch.cuda.synchronize()
    assert not out.any()                                   # capturing ran nothing
    for ua, fb in imgs[1:]:
        a.copy_(_dev(ua))
        b[..., :3] = _dev(fb).to(torch.bfloat16)
        graph.replay()
        torch.cuda.synchronize()
        eager = K.image_quality(a.clone(), b.clone())
        assert np.array_equal(_bits(out), _bits(eager)) and not np.array_equal(_bits(out), _bits(warm))
        _check(out, ua, b[..., :3].float().cpu().numpy(), "replay")


# ---- metric.py ---------------------------------------------------------------------------------------------------------------
def test_metric_image_quality_takes_numpy_torch_and_generator_outputs():
    from sggan_amd.model import _LazyUnpad
    H, W = 15, 21
    a = _u8((2, H, W, 3), 71)
    x = _float_image((2, H, W, 3), 72, False)
    want = O.scores(a, x)
    got = M.image_quality(a, x)                            # NumPy in
    assert set(got) == {"MAE", "MSE", "PSNR", "SSIM"}
    for k in ("MAE", "MSE", "PSNR"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0)
    assert np.abs(got["SSIM"] - want["SSIM"]).max() <= SSIM_ATOL
    pad = K.pad_channels(_dev(x), A.CPAD, torch.float32)
    for other in (_dev(x), pad, _LazyUnpad(pad, 3)):       # torch, the internal layout, a lazy generator output
        again = M.image_quality(_dev(a), other)
        assert all(np.array_equal(again[k], got[k]) for k in got)
    one = M.image_quality(a[0], x[0])                      # (H,W,C) -> one image
    assert all(one[k].shape == (1,) and one[k][0] == got[k][0] for k in got)
    same = M.image_quality(a, a)
    assert np.isinf(same["PSNR"]).all() and np.array_equal(same["SSIM"], [1.0, 1.0]) and not same["MAE"].any()
    acc = M.scores_image_fake(a, a)
    assert len(acc) == 1 and acc[0][0].is_cuda and M.scores_image_fake(a[:1], x[:1], acc) is acc and len(acc) == 2
    s = M.scores_from_quality(M.scores_image_fake(a, a))
    assert s["MAE"] == 0.0 and s["SSIM"] == 1.0 and s["PSNR"] == 10.0 * np.log10(255.0 ** 2 * (2 * 3 * H * W))
    with pytest.raises(ValueError):
        M.scores_from_quality([])


# ---- the test passes ---------------------------------------------------------------------------------------------------------
REF_TAGS = ["Overall Accuracy", "Mean Accuracy", "Frequency Weighted Accuracy", "Mean IoU"]
CLASS_TAGS = ["Class " + t for t in REF_TAGS] + ["Boundary Class Mean IoU"]
IMAGE_TAGS = ["Image MAE", "Image PSNR", "Image SSIM"]
CYCLE_TAGS = ["Cycle MAE", "Cycle PSNR", "Cycle SSIM"]
SIDE = 32


def _args(**kw):
    return sggan_amd.default_args(**dict(dict(ngf=8, ndf=8, n_blocks=2, dtype="f32", image_height=SIDE, image_width=SIDE, test_dir=None), **kw))


def _samples(a):
    from sggan_amd.main import synthetic_test_samples
    return list(synthetic_test_samples(a, 2)())


def _run(model, **kw):
    from sggan_amd.utils import SummarySink
    a = _args(**kw)
    sink = SummarySink()
    fakes, score = model.test_during_train(4, a, _samples(a), sink)
    return a, sink.records, fakes, score


def _target(seg_image):
    from sggan_amd.utils import convert_image_dtype_uint8
    return convert_image_dtype_uint8(np.asarray(seg_image)[None]).astype(np.uint8)


def _want_from_files(a, folder):
    from PIL import Image
    rows = []
    for name, _, seg in (s[:3] for s in _samples(a)):
        png = np.asarray(Image.open(os.path.join(folder, os.path.basename(name))), dtype=np.uint8)
        assert png.shape == (SIDE, SIDE, 3)
        rows.append(O.sums(_target(seg), png[None])[0])
    return O.pooled(rows, SIDE, SIDE)


def _assert_scores(got, want):
    assert abs(got["MAE"] - want["MAE"]) <= 1e-12 * abs(want["MAE"]), (got["MAE"], want["MAE"])
    assert abs(got["PSNR"] - want["PSNR"]) <= 1e-12 * abs(want["PSNR"]), (got["PSNR"], want["PSNR"])
    assert abs(got["SSIM"] - want["SSIM"]) <= SSIM_ATOL, (got["SSIM"], want["SSIM"])


@pytest.fixture(scope="module")
def plain_model():
    return sggan_amd.sggan(_args())


def test_test_during_train_logs_the_image_scalars_of_the_files_it_wrote(plain_model, tmp_path):
    base_a, base, _, base_score = _run(plain_model)
    assert [r["tag"] for r in base] == REF_TAGS and "Image" not in base_score
    a, rec, fakes, score = _run(plain_model, image_scores=True, test_dir=str(tmp_path / "out"))
    assert [r["tag"] for r in rec] == REF_TAGS + IMAGE_TAGS and all(r["step"] == 4 for r in rec)        # a non-cycle model: no Cycle ...
    assert "Cycle" not in score
    want = _want_from_files(a, str(tmp_path / "out"))
    got = {r["tag"]: r["value"] for r in rec}
    print("Image", {k: got["Image " + k] for k in want}, "files", want)
    _assert_scores({k: got["Image " + k] for k in want}, want)
    assert all(score["Image"][k] == got["Image " + k] for k in want) and want["MAE"] > 0 and np.isfinite(want["PSNR"])
    assert set(score["Image"]) == {"MAE", "PSNR", "SSIM", "per_image"} and score["Image"]["per_image"]["SSIM"].shape == (2,)
    # without the flag: the records and scores of a run with it, minus the new entries
    assert rec[:4] == base
    np.testing.assert_equal({k: v for k, v in score.items() if k != "Image"}, base_score)
    off = _run(plain_model, image_scores=False)
    assert off[1] == base
    np.testing.assert_equal(off[3], base_score)


def test_image_scalars_follow_the_class_scalars_and_ema_decay_stays_last(tmp_path):
    m = sggan_amd.sggan(_args(ema_decay=0.5))
    kw = dict(class_scores=True, segment_class=34)
    _, base, _, base_score = _run(m, **kw)
    assert [r["tag"] for r in base] == REF_TAGS + CLASS_TAGS + ["EMA Decay"]
    a, rec, _, score = _run(m, image_scores=True, test_dir=str(tmp_path / "out"), **kw)
    assert [r["tag"] for r in rec] == REF_TAGS + CLASS_TAGS + IMAGE_TAGS + ["EMA Decay"]
    assert [r for r in rec if r["tag"] not in IMAGE_TAGS] == base
    np.testing.assert_equal({k: v for k, v in score.items() if k != "Image"}, base_score)
    _assert_scores(score["Image"], _want_from_files(a, str(tmp_path / "out")))


def test_cycle_model_also_scores_the_reconstruction_against_the_input():
    from sggan_amd.utils import convert_image_dtype_uint8
    m = sggan_amd.sggan(_args(cycle=True))
    a, rec, _, score = _run(m, image_scores=True)
    assert [r["tag"] for r in rec] == REF_TAGS + IMAGE_TAGS + CYCLE_TAGS
    rows = []
    for _, sample, _ in _samples(a):
        rescaled = convert_image_dtype_uint8(np.asarray(sample)[None])
        back = m.generator_BA(m.generator(torch.as_tensor(rescaled).to(m.device)))
        rows.append(O.sums(rescaled.astype(np.uint8), back.cpu().numpy())[0])
    want = O.pooled(rows, SIDE, SIDE)
    got = {r["tag"]: r["value"] for r in rec}
    print("Cycle", {k: got["Cycle " + k] for k in want}, "direct", want)
    _assert_scores({k: got["Cycle " + k] for k in want}, want)
    assert all(score["Cycle"][k] == got["Cycle " + k] for k in want)
    _, off, _, off_score = _run(m)
    assert [r["tag"] for r in off] == REF_TAGS and off == rec[:4] and "Cycle" not in off_score and "Image" not in off_score


def test_phase_test_logs_one_line_with_the_three_values_of_the_files(plain_model, tmp_path):
    import re
    a = _args(image_scores=True, checkpoint_dir=str(tmp_path / "ckpt"))
    a.test_dir = str(tmp_path / "out")
    lines = []
    plain_model.test(a, _samples(a), log=lines.append)
    m = re.fullmatch(r"Image MAE: (\S+) Image PSNR: (\S+) Image SSIM: (\S+)", lines[-1])
    assert m and sum("Image MAE" in l for l in lines) == 1
    want = _want_from_files(a, a.test_dir)
    for value, key in zip(m.groups(), ("MAE", "PSNR", "SSIM")):
        assert abs(float(value) - want[key]) <= 1e-6, (key, value, want[key])             # (%f prints six decimals)
    b = _args(checkpoint_dir=str(tmp_path / "ckpt"))
    b.test_dir = str(tmp_path / "out")
    bare = []
    plain_model.test(b, _samples(b), log=bare.append)
    assert bare == lines[:-1]
    two = []                                                # samples without a label image: nothing to score
    plain_model.test(a, [s[:2] for s in _samples(a)], log=two.append)
    assert two == bare
