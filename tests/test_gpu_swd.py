"""The sliced Wasserstein distance of the test pass on the GPU (csrc/swd.hip, metric.SWD) against the float64
oracle of tests/swd_oracle.py.

Bounds.  The pyramid and the descriptors are compared with ``array_equal``: with 8-bit inputs every intermediate of the pyramid
is an exact dyadic rational and the float32 store its one rounding.  Projections and scores are sums of rounded products;
eps64 (tests/golden/swd_eps.json) is the worst difference of the float64 oracle from the same oracle in np.longdouble on these
inputs -- the error of the number format -- and the GPU must lie within 16 * eps64 of the oracle: projections relative to
sum_k |z_k d_k|, scores relative to the score.  The factor covers the other order of the chunked sums; the sort is 1-Lipschitz
in the maximum norm and adds nothing."""
import math
import os
import re

import numpy as np
import pytest
import torch

import sggan_amd
from sggan_amd import kernels as K
from sggan_amd import metric as M
from tests import swd_oracle as O

pytestmark = pytest.mark.gpu

PYRAMID_CASES = {"16x16x1": (1, 16, 16, 1), "32x48x2": (1, 32, 48, 2), "64x96x3": (3, 64, 96, 3), "112x176x5": (1, 112, 176, 5)}
KINDS = ["u8x3", "u8x4", "f32x3", "bf16x8"]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _image(name, kind):
    """-> (device operand, what the oracle reads).  Float operands carry -1, 1, values past both and a NaN."""
    N, H, W, _ = PYRAMID_CASES[name]
    rng = np.random.default_rng(len(name) * 131 + KINDS.index(kind))
    u8 = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    if kind == "u8x3":
        return _dev(u8), u8
    if kind == "u8x4":
        return _dev(np.concatenate([u8, rng.integers(0, 256, (N, H, W, 1)).astype(np.uint8)], axis=-1)), u8
    x = (u8.astype(np.float32) + rng.uniform(0.05, 0.95, u8.shape).astype(np.float32)) / np.float32(127.5) - np.float32(1)
    x[0, 0, :6, 0] = [-1.0, 1.0, -3.0, 7.0, np.nan, 0.0]
    x[-1, -1, -1] = [np.nan, 1.0, -1.0]
    if kind == "f32x3":
        return _dev(x), x
    t = torch.as_tensor(np.concatenate([x, rng.uniform(-2, 2, (N, H, W, 5)).astype(np.float32)], axis=-1)).to(torch.bfloat16).cuda()
    return t, t[..., :3].float().cpu().numpy()


# ------------------------------------------------------------------------------------------------ pyramid
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", PYRAMID_CASES)
def test_pyramid_equals_the_oracle_rounded_to_float32(name, kind):
    N, H, W, levels = PYRAMID_CASES[name]
    dev, host = _image(name, kind)
    got = K.swd_pyramid(dev, levels)
    want = O.pyramid_flat(host, levels)
    assert tuple(got.shape) == want.shape == (N, K.swd_pyramid_elems(H, W, levels)) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want)
    if N > 1:                                              # image n of a batch: the bits of the call on that image alone
        for n in range(N):
            assert torch.equal(K.swd_pyramid(dev[n:n + 1].contiguous(), levels)[0], got[n])
    assert torch.equal(K.swd_pyramid(dev, levels), got)


def test_quantisation_is_the_rule_of_the_saved_image():
    """Level 0 of a one-level pyramid is the 8-bit image itself: the float operand gives the bytes save_images would write."""
    dev, host = _image("16x16x1", "f32x3")
    got = K.swd_pyramid(dev, 1).cpu().numpy().reshape(1, 3, 16, 16)
    q = O.quantise(host)
    assert np.array_equal(got, q.transpose(0, 3, 1, 2).astype(np.float32))
    assert q[0, 0, :6, 0].tolist() == [0, 255, 0, 255, 0, 127]


# ------------------------------------------------------------------------------------------------ descriptors
@pytest.fixture(scope="module")
def big():
    N, H, W, levels = 3, 112, 176, 5
    u8 = np.random.default_rng(11).integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    pyr = K.swd_pyramid(_dev(u8), levels)
    planar = [l.astype(np.float32) for l in O.pyramid(u8, levels)]
    assert np.array_equal(pyr.cpu().numpy(), O.pyramid_flat(u8, levels))
    return dict(N=N, H=H, W=W, levels=levels, pyr=pyr, planar=planar)


def _desc(big, level, patches, offset, rows=slice(None)):
    pyr = big["pyr"][rows].contiguous()
    out = torch.full((pyr.shape[0] * patches, K.SWD_K), float("nan"), dtype=torch.float32, device="cuda")
    return K.swd_descriptors(pyr, big["H"], big["W"], big["levels"], level, patches, 19, offset, out)


@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("patches", [1, 2, 33])
def test_descriptors_equal_the_oracle_at_every_level(big, patches, offset):
    for level in range(big["levels"]):
        got = _desc(big, level, patches, offset).cpu().numpy()
        want = O.descriptors(big["planar"][level], level, patches, 19, offset)
        assert got.shape == want.shape == (3 * patches, 147) and np.array_equal(got, want), level


def test_a_batch_of_three_equals_three_calls_at_offsets_0_1_2(big):
    for level in (0, 4):
        whole = _desc(big, level, 33, 0)
        for n in range(3):
            assert torch.equal(_desc(big, level, 33, n, slice(n, n + 1)), whole[n * 33:(n + 1) * 33])
        assert not torch.equal(_desc(big, level, 33, 1, slice(0, 1)), whole[:33])            # keyed by the image index


# ------------------------------------------------------------------------------------------------ projection, moments, score
@pytest.fixture(scope="module")
def eps():
    return O.golden_eps64()


def _gpu_score(a, b, dirs):
    pa, ma = K.swd_project(a, dirs)
    pb, mb = K.swd_project(b, dirs)
    sums = K.swd_distance(torch.sort(pa, dim=1).values, torch.sort(pb, dim=1).values)
    D, Mr = pa.shape
    return pa, ma, pb, mb, sums, 1e3 * math.fsum(sums.cpu().numpy()) / (float(D) * float(Mr))


@pytest.mark.parametrize("M_rows,D", O.SCORE_CASES)
def test_projection_moments_and_score_within_16_eps64_of_the_oracle(M_rows, D, eps):
    a, b = O.case_descriptors(M_rows, D)
    dirs = O.directions(D)
    assert np.array_equal(M.swd_directions(D).numpy(), dirs)
    pa, ma, pb, mb, sums, got = _gpu_score(_dev(a), _dev(b), _dev(dirs))
    assert tuple(pa.shape) == (D, M_rows) and pa.dtype == torch.float64 and tuple(ma.shape) == (3, 2)
    for desc, p, m in ((a, pa, ma), (b, pb, mb)):
        want_m = O.moments(desc)
        scale = np.abs(desc.astype(np.float64)).reshape(M_rows, 3, 49).mean(axis=(0, 2))
        m = m.cpu().numpy()
        err_mean, err_std = np.abs(m[:, 0] - want_m[:, 0]) / scale, np.abs(m[:, 1] - want_m[:, 1]) / want_m[:, 1]
        want_p, mag = O.project(O.normalise(desc), dirs)
        err = float((np.abs(p.cpu().numpy() - want_p) / mag).max())
        print(f"M={M_rows} D={D}: mean {err_mean.max():.2e} std {err_std.max():.2e} proj {err:.2e}, bound {16 * eps['proj']:.2e}")
        assert err_mean.max() <= 16 * eps["proj"] and err_std.max() <= 16 * eps["proj"]
        assert err <= 16 * eps["proj"]
    want = float(O.score(a, b, dirs))
    print(f"M={M_rows} D={D}: score {got!r} oracle {want!r} rel {abs(got - want) / want:.2e}, bound {16 * eps['score']:.2e}")
    assert want > 0 and abs(got - want) <= 16 * eps["score"] * want
    # the same call again: the same bits, down to the per-direction sums
    again = _gpu_score(_dev(a), _dev(b), _dev(dirs))
    assert torch.equal(again[0], pa) and torch.equal(again[2], pb) and torch.equal(again[4], sums) and again[5] == got
    # identical sets: exactly zero
    assert _gpu_score(_dev(a), _dev(a.copy()), _dev(dirs))[5] == 0.0


def test_full_score_of_an_image_set_within_16_eps64_of_the_oracle(eps):
    c = O.image_case()
    kw = {k: c[k] for k in ("levels", "patches", "repeats", "dirs_per_repeat", "seed")}
    res = M.sliced_wasserstein(c["fakes"], c["reals"], **kw)
    dirs = O.directions(c["repeats"] * c["dirs_per_repeat"], c["seed"])
    vals, mean = O.swd(c["fakes"], c["reals"], c["levels"], c["patches"], dirs, c["seed"])
    assert [(h, w) for h, w, _ in res["levels"]] == [(32, 48), (16, 24)]
    for (_, _, got), want in list(zip(res["levels"], vals)) + [((0, 0, res["mean"]), mean)]:
        print(f"score {got!r} oracle {float(want)!r} rel {abs(got - want) / want:.2e}, bound {16 * eps['score']:.2e}")
        assert abs(got - want) <= 16 * eps["score"] * want
    assert M.sliced_wasserstein(c["fakes"], c["reals"], **kw) == res
    # uint8 with four channels and the float image of the same colours give the same bits
    rgba = np.concatenate([c["fakes"], np.zeros_like(c["fakes"][..., :1])], axis=-1)
    assert M.sliced_wasserstein(rgba, c["reals"], **kw) == res
    as_float = ((c["fakes"].astype(np.float32) + np.float32(0.5)) / np.float32(127.5) - np.float32(1)).astype(np.float32)
    assert np.array_equal(O.quantise(as_float), c["fakes"]) and M.sliced_wasserstein(as_float, c["reals"], **kw) == res
    # identical sets: exactly zero; one constant channel: finite and the oracle's
    same = M.sliced_wasserstein(c["reals"], c["reals"].copy(), **kw)
    assert [v for _, _, v in same["levels"]] == [0.0, 0.0] and same["mean"] == 0.0
    one = c["reals"].copy()
    one[..., 1] = 200
    got = M.sliced_wasserstein(one, c["fakes"], **kw)
    vals, mean = O.swd(one, c["fakes"], c["levels"], c["patches"], dirs, c["seed"])
    assert np.isfinite(got["mean"]) and abs(got["mean"] - mean) <= 16 * eps["score"] * mean
    for (_, _, g), w in zip(got["levels"], vals):
        assert np.isfinite(g) and abs(g - w) <= 16 * eps["score"] * w
    const = np.full((3, 32, 48, 3), 77, np.uint8)          # every deviation zero: 0.0, not NaN
    flat = M.sliced_wasserstein(const, const, **kw)
    assert flat["mean"] == 0.0 and [v for _, _, v in flat["levels"]] == [0.0, 0.0]


def test_batching_does_not_change_a_bit():
    rng = np.random.default_rng(5)
    fakes, reals = (rng.integers(0, 256, (6, 32, 48, 3)).astype(np.uint8) for _ in range(2))
    kw = dict(patches=11, repeats=2, dirs_per_repeat=16, levels=2)
    results = []
    for step in (1, 3, 6):
        s = M.SWD(32, 48, 6, **kw)
        for i in range(0, 6, step):
            s.add(fakes[i:i + step], reals[i:i + step])
        results.append(s.result())
    assert results[0] == results[1] == results[2] and results[0]["mean"] > 0
    # the two sets filled independently, the reals first, and more fakes than reals: the smaller count is used by both
    s = M.SWD(32, 48, 6, **kw)
    s.add_reals(reals[:4])
    s.add_fakes(fakes)
    t = M.SWD(32, 48, 4, **kw)
    t.add(fakes[:4], reals[:4])
    assert s.count == {"fakes": 6, "reals": 4} and s.result() == t.result() and s.result() != results[0]
    with pytest.raises(ValueError):
        s.add_fakes(fakes[:1])                              # past n_max
    with pytest.raises(ValueError):
        M.SWD(12, 64, 2)                                    # no level: the message names the rule
    with pytest.raises(ValueError):
        M.SWD(32, 48, 2).result()                           # an empty set


# ------------------------------------------------------------------------------------------------ the test passes
REF_TAGS = ["Overall Accuracy", "Mean Accuracy", "Frequency Weighted Accuracy", "Mean IoU"]
SWD_TAGS = ["SWD 128x128", "SWD 64x64", "SWD 32x32", "SWD 16x16", "SWD Mean"]
SIDE = 128


def _args(**kw):
    return sggan_amd.default_args(**dict(dict(ngf=8, ndf=8, n_blocks=2, dtype="f32", image_height=SIDE, image_width=SIDE, test_dir=None), **kw))


def _samples(a):
    from sggan_amd.main import synthetic_test_samples
    return list(synthetic_test_samples(a, 2)())


def _run(model, swd_reals=None, **kw):
    from sggan_amd.utils import SummarySink
    a = _args(**kw)
    sink = SummarySink()
    extra = {} if swd_reals is None else {"swd_reals": swd_reals}
    fakes, score = model.test_during_train(4, a, _samples(a), sink, **extra)
    return a, sink.records, fakes, score


def _u8(img01):
    from sggan_amd.utils import convert_image_dtype_uint8
    return convert_image_dtype_uint8(np.asarray(img01)[None]).astype(np.uint8)


def _saved(a, folder):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(folder, os.path.basename(s[0]))), dtype=np.uint8) for s in _samples(a)])


def _check_scalars(rec, score, want):
    got = {r["tag"]: r["value"] for r in rec}
    assert [got[t] for t in SWD_TAGS] == [v for _, _, v in want["levels"]] + [want["mean"]]
    assert score["SWD"] == want and want["mean"] > 0 and [(h, w) for h, w, _ in want["levels"]] == [(128, 128), (64, 64), (32, 32), (16, 16)]


def test_reference_mode_test_pass_scores_the_files_it_wrote_against_the_labels(tmp_path):
    model = sggan_amd.sggan(_args())
    base_a, base, _, base_score = _run(model)
    assert [r["tag"] for r in base] == REF_TAGS and "SWD" not in base_score           # without the flag: today's scalars
    a, rec, _, score = _run(model, swd=True, swd_patches=16, test_dir=str(tmp_path / "out"))
    assert [r["tag"] for r in rec] == REF_TAGS + SWD_TAGS and all(r["step"] == 4 for r in rec)
    labels = np.concatenate([_u8(s[2]) for s in _samples(a)])
    want = M.sliced_wasserstein(_saved(a, a.test_dir), labels, patches=16)
    _check_scalars(rec, score, want)
    assert rec[:4] == base
    np.testing.assert_equal({k: v for k, v in score.items() if k != "SWD"}, base_score)
    off = _run(model, swd=False)
    assert off[1] == base
    # a model that keeps a weight average: its 'EMA Decay' stays the last scalar
    ema = sggan_amd.sggan(_args(ema_decay=0.5))
    _, ema_base, _, _ = _run(ema)
    _, ema_rec, _, _ = _run(ema, swd=True, swd_patches=16)
    assert [r["tag"] for r in ema_base] == REF_TAGS + ["EMA Decay"] and [r["tag"] for r in ema_rec] == REF_TAGS + SWD_TAGS + ["EMA Decay"]
    assert [r for r in ema_rec if r["tag"] not in SWD_TAGS] == ema_base
    # --phase test: one line with the same values
    b = _args(swd=True, swd_patches=16, checkpoint_dir=str(tmp_path / "ckpt"))
    b.test_dir = str(tmp_path / "out2")
    lines = []
    model.test(b, _samples(b), log=lines.append)
    assert sum("SWD Mean" in l for l in lines) == 1
    m = re.fullmatch(r"SWD 128x128: (\S+) SWD 64x64: (\S+) SWD 32x32: (\S+) SWD 16x16: (\S+) SWD Mean: (\S+)", lines[-1])
    assert m
    for value, w in zip(m.groups(), [v for _, _, v in want["levels"]] + [want["mean"]]):
        assert abs(float(value) - w) <= 1e-6, (value, w)                                 # (%f prints six decimals)
    bare = []
    c = _args(checkpoint_dir=str(tmp_path / "ckpt"))
    c.test_dir = str(tmp_path / "out2")
    model.test(c, _samples(c), log=bare.append)
    assert bare == lines[:-1]


def test_cycle_model_scores_against_the_unpaired_reals(tmp_path):
    model = sggan_amd.sggan(_args(cycle=True))
    rng = np.random.default_rng(9)
    reals = [rng.uniform(0, 1, (SIDE, SIDE, 3)).astype(np.float32) for _ in range(3)]     # one more than there are fakes
    _, base, _, base_score = _run(model)
    assert [r["tag"] for r in base] == REF_TAGS
    a, rec, _, score = _run(model, swd_reals=lambda: iter(reals), swd=True, swd_patches=16, test_dir=str(tmp_path / "out"))
    assert [r["tag"] for r in rec] == REF_TAGS + SWD_TAGS
    want = M.sliced_wasserstein(_saved(a, a.test_dir), np.concatenate([_u8(r) for r in reals[:2]]), patches=16)
    _check_scalars(rec, score, want)
    assert [r for r in rec if r["tag"] not in SWD_TAGS] == base
    labels = M.sliced_wasserstein(_saved(a, a.test_dir), np.concatenate([_u8(s[2]) for s in _samples(a)]), patches=16)
    assert labels != want                                   # the given reals were used, not the label images


# ------------------------------------------------------------------------------------------------ the reals of a dataset directory
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "city_small")


def test_cycle_mode_on_a_dataset_directory_takes_the_reals_from_domain_b(tmp_path):
    """--swd --cycle: the first n images, in sorted order, of testB (else trainB) of the domain-B root, through the test samples'
    own resize; every other case leaves ``args.swd_reals`` unset (the label images are the reals)."""
    import shutil
    from sggan_amd import data as D
    from sggan_amd.main import parse_args, set_swd_reals
    root = tmp_path / "b"
    shutil.copytree(os.path.join(FIX, "trainA"), root / "trainB")
    size = ["--img_height", "32", "--img_width", "64"]
    a = parse_args(["--swd", "--cycle", "--dataset_dir", FIX, "--dataset_dir_B", str(root)] + size)
    set_swd_reals(a, "cuda", 1)
    got = list(a.swd_reals())
    assert len(got) == 1 and got[0].shape == (32, 64, 3) and got[0].dtype == np.float32
    want = list(D.directory_test_samples(a, D.DatasetCache(FIX, "trainA", with_class=False))())
    assert np.array_equal(got[0], want[0][1])                                       # aachen_000000: the first in sorted order
    set_swd_reals(a, "cuda", 5)                                                     # more asked for than there are: all of them
    both = list(a.swd_reals())
    assert len(both) == 2 and np.array_equal(both[0], want[0][1]) and np.array_equal(both[1], want[1][1])
    shutil.copytree(os.path.join(FIX, "testA"), root / "testB")                     # testB wins over trainB
    set_swd_reals(a, "cuda", 5)
    test_b = list(a.swd_reals())
    assert len(test_b) == 1 and not np.array_equal(test_b[0], want[0][1])
    # the yielded images go into the score as the 8-bit images of everything else
    s = M.SWD(32, 64, 2, patches=4, repeats=1, dirs_per_repeat=8)
    sggan_amd.sggan._swd_add_reals(s, a.swd_reals)                                  # no fakes yet: none are taken
    assert s.count["reals"] == 0
    s.add_fakes(np.concatenate([_u8(x) for x in both]))
    sggan_amd.sggan._swd_add_reals(s, a.swd_reals)
    assert s.count == {"fakes": 2, "reals": 1}
    for argv in (["--swd", "--dataset_dir", FIX], ["--cycle", "--dataset_dir", FIX, "--dataset_dir_B", str(root)],
                 ["--swd", "--cycle", "--dataset_dir", FIX]):                       # reference mode / no flag / no domain-B folder
        b = parse_args(argv + size)
        set_swd_reals(b, "cuda", 2)
        assert not hasattr(b, "swd_reals")
