"""Augmented training copy, host side (no GPU): the warp's rule stated twice, its known answers, the epoch plan's second
random stream, the ABI entries, the new kernels' build resources and the command line."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import sggan_amd  # noqa: F401
from sggan_amd import _abi as A
from sggan_amd import data as D

from tests import augment_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "city_small")


def _params(**kw):
    p = D.identity_augment_params(1)
    for k, v in kw.items():
        p[k] = np.asarray([v], dtype=p[k].dtype)
    return p


def test_composite_matrices_equal_the_sequential_oracle():
    """data.apply_augment (two composite matrices) against tests/augment_oracle.py (sequential maps) for all six orders, with
    drawn parameters and with both ends of every range; the cases include zero-filled and fill-free ones."""
    S = 48
    rng = np.random.default_rng(0)
    img = rng.random((S, S, 3))
    drawn = D.draw_augment_params(np.random.RandomState(4), 12)
    sets = AO.extremes() + [dict(AO.one(drawn, i), perm=list(perm)) for i, perm in
                            enumerate(list(itertools.permutations(range(3))) * 2)]
    mats = D.augment_matrices(AO.stack(sets), S)
    assert mats.shape == (len(sets), 2, 2, 3) and mats.dtype == np.float64
    filled, worst = [], 0.0
    for p, m in zip(sets, mats):
        want, inside = AO.warp(img, p)
        got = D.apply_augment(img, m)
        worst = max(worst, np.abs(got - want).max())
        filled.append(not inside.all())
        assert np.array_equal(got[~inside], np.zeros_like(got[~inside]))
    print(f"{len(sets)} parameter sets, {sum(filled)} with zero fill, max |composite - sequential| {worst:.3e}")
    assert worst <= 1e-12
    assert any(filled) and not all(filled)
    assert {tuple(p["perm"]) for p in sets} == set(itertools.permutations(range(3)))


def test_identity_parameters_return_the_image():
    img = np.random.default_rng(1).random((20, 20, 4))
    for perm in itertools.permutations(range(3)):
        m = D.augment_matrices(_params(perm=perm), 20)[0]
        assert np.array_equal(m[0], np.eye(3)[:2]) and np.array_equal(m[1], np.eye(3)[:2])
        assert np.array_equal(D.apply_augment(img, m), img)


def test_known_answers():
    S = 8
    img = np.random.default_rng(2).integers(0, 256, (S, S, 2)).astype(np.float64)
    # flip only
    got = D.apply_augment(img, D.augment_matrices(_params(flip=True), S)[0])
    assert np.array_equal(got, img[:, ::-1])
    # crop only: 2 pixels off every side keeps 4 of 8, an exact 2x bilinear upscale: output centre x + 0.5 samples the squared
    # image at 2 + (x + 0.5) / 2, i.e. between pixels floor(u), floor(u) + 1 with u = 1.75 + x / 2
    got = D.apply_augment(img, D.augment_matrices(_params(crop=[0.25, 0.25, 0.25, 0.25]), S)[0])
    for y, x in ((0, 0), (3, 5), (7, 7), (2, 1)):
        u, v = 1.75 + x / 2.0, 1.75 + y / 2.0
        x0, y0, fx, fy = int(u), int(v), u - int(u), v - int(v)
        want = ((1 - fy) * (1 - fx)) * img[y0, x0] + ((1 - fy) * fx) * img[y0, x0 + 1] + (fy * (1 - fx)) * img[y0 + 1, x0] + (fy * fx) * img[y0 + 1, x0 + 1]
        assert np.array_equal(got[y, x], want), (y, x)
    assert np.array_equal(got[0, 0], (img[1, 1] + 3 * img[1, 2] + 3 * img[2, 1] + 9 * img[2, 2]) / 16)   # u = v = 1.75
    # unequal sides: rounding to whole pixels (0.3 * 8 = 2.4 -> 2, 0.2 * 8 = 1.6 -> 2)
    a = D.augment_matrices(_params(crop=[0.3, 0.2, 0.2, 0.3]), S)[0]
    b = D.augment_matrices(_params(crop=[0.25, 0.25, 0.25, 0.25]), S)[0]
    assert np.array_equal(a, b)
    # translation by whole pixels: +2 columns, -1 row; the vacated columns and row are zero
    got = D.apply_augment(img, D.augment_matrices(_params(translate=[0.25, -0.125]), S)[0])
    want = np.zeros_like(img)
    want[:S - 1, 2:] = img[1:, :S - 2]
    assert np.array_equal(got, want)
    assert not got[:, :2].any() and not got[S - 1].any()


def test_zero_fill_is_decided_in_the_affine_frame():
    """Crop applied AFTER the affine looks at its interior only (no fill: every pixel is 1 up to the rounding of four weights that sum to 1);
    applied before, the fill survives."""
    S = 40
    img = np.ones((S, S, 1))
    kw = dict(translate=[0.1, 0.1], crop=[0.2, 0.2, 0.2, 0.2])
    after = D.apply_augment(img, D.augment_matrices(_params(perm=[D.AUG_AFFINE, D.AUG_CROP, D.AUG_FLIP], **kw), S)[0])
    before = D.apply_augment(img, D.augment_matrices(_params(perm=[D.AUG_CROP, D.AUG_AFFINE, D.AUG_FLIP], **kw), S)[0])
    assert np.abs(after - 1.0).max() <= 4e-16 and before[:4, :4].max() == 0.0 and before[S // 2, S // 2] == 1.0


class _StubDomain:
    def __init__(self, n):
        self.cache = list(range(n))


def _loader(augment, n_files, batch, seed=5, aug_seed=23, domains=1):
    b = D.DirectoryBatches.__new__(D.DirectoryBatches)
    b.args = SimpleNamespace(batch_size=batch, train_size=10 ** 8)
    b.rng, b.aug_rng, b.augment = np.random.RandomState(seed), np.random.RandomState(aug_seed), augment
    b.domains = [_StubDomain(n_files) for _ in range(domains)]
    return b


def test_plan_is_deterministic_and_leaves_the_plain_stream_alone():
    plain, aug, again = _loader(False, 10, 3), _loader(True, 10, 3), _loader(True, 10, 3)
    for _ in range(3):
        o0, f0, n0 = plain.epoch_plan()
        o1, f1, n1 = aug.epoch_plan()
        o2, f2, n2 = again.epoch_plan()
        p1, p2 = aug.augment_plan(o1), again.augment_plan(o2)
        assert o0 == o1 == o2 and np.array_equal(f0, f1) and n0 == n1 == n2 == 3
        assert len(p1) == 1 and all(np.array_equal(p1[0][k], p2[0][k]) for k in p1[0])
        p = p1[0]
        assert p["perm"].shape == (9, 3) and all(sorted(r) == [0, 1, 2] for r in p["perm"].tolist())
        assert p["crop"].shape == (9, 4) and p["crop"].min() >= 0.2 and p["crop"].max() <= 0.4
        assert p["translate"].shape == (9, 2) and np.abs(p["translate"]).max() <= 0.1 and np.abs(p["angle"]).max() <= 1.0
        assert p["flip"].dtype == p["loader_flip"].dtype == np.bool_
    assert plain.rng.random_sample() == aug.rng.random_sample()              # the first stream stands where it stood
    other, same = _loader(True, 10, 3, aug_seed=24), _loader(True, 10, 3)
    oo, os_ = other.epoch_plan()[0], same.epoch_plan()[0]
    assert oo == os_ and not np.array_equal(other.augment_plan(oo)[0]["crop"], same.augment_plan(os_)[0]["crop"])
    # two domains: A's parameters are drawn first, then B's, from the one second stream
    l2 = _loader(True, 6, 2, domains=2)
    two = l2.augment_plan(l2.epoch_plan()[0])
    ref = np.random.RandomState(23)
    for got in two:
        want = D.draw_augment_params(ref, 6)
        assert all(np.array_equal(got[k], want[k]) for k in want)


def test_draw_order_is_the_documented_one():
    got = D.draw_augment_params(np.random.RandomState(7), 2)
    r = np.random.RandomState(7)
    for i in range(2):
        assert np.array_equal(got["perm"][i], r.permutation(3))
        assert got["flip"][i] == (r.random_sample() < 0.5)
        assert np.array_equal(got["crop"][i], [r.uniform(0.2, 0.4) for _ in range(4)])            # top, right, bottom, left
        assert np.array_equal(got["translate"][i], [r.uniform(-0.1, 0.1) for _ in range(2)])
        assert got["angle"][i] == r.uniform(-1.0, 1.0)
        assert got["loader_flip"][i] == (r.random_sample() > 0.5)


def test_doubled_batch_layout_is_interleaved():
    """Rows of the doubled batch: file f twice in a row, the plain flip then the copy's; per-sample matrices use the side of
    the sample's own source."""
    assert D.interleave(np.array([1, 0, 1]), np.array([0, 0, 1])).tolist() == [1, 0, 0, 0, 1, 1]
    cache = D.DatasetCache(FIX, "trainA", device="cpu")
    stub = SimpleNamespace(cache=cache)
    aug = D.draw_augment_params(np.random.RandomState(23), 2)
    plan = D._Domain.plan(stub, [1, 0], aug)
    assert plan["file2"].tolist() == [1, 1, 0, 0] and plan["file"].tolist() == [1, 0]
    want = D.augment_matrices(aug, 512)
    assert np.array_equal(plan["img_mats"].numpy(), want) and np.array_equal(plan["lab_mats"].numpy(), want)
    # the warp's window is the bound over the parameter ranges, the same whatever was drawn
    assert plan["img_win"] == plan["lab_win"] == D.warp_window_bound(512) == (14, 43)
    assert all(a <= b for a, b in zip(D.warp_window(want), plan["img_win"]))
    assert "file2" not in D._Domain.plan(stub, [1, 0])


def test_warp_window_covers_every_neighbour():
    """The LDS window data.warp_window sizes holds all four neighbours of every pixel of every 16 x 64 tile."""
    S = 160
    sets = AO.extremes()
    mats = D.augment_matrices(AO.stack(sets), S)
    wh, ww = D.warp_window(mats)
    assert all(a <= b for a, b in zip((wh, ww), D.warp_window_bound(S)))         # both ends of every range are inside the bound
    for p in sets:
        x, y, _ = AO.source_points(p, S)
        x0, y0 = np.clip(np.floor(x - 0.5), 0, S - 1), np.clip(np.floor(y - 0.5), 0, S - 1)
        x1, y1 = np.clip(np.floor(x - 0.5) + 1, 0, S - 1), np.clip(np.floor(y - 0.5) + 1, 0, S - 1)
        for ty in range(0, S, 16):
            for tx in range(0, S, 64):
                t = (slice(ty, ty + 16), slice(tx, tx + 64))
                assert x1[t].max() - x0[t].min() + 1 <= ww and y1[t].max() - y0[t].min() + 1 <= wh


def test_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sggan.h")).read(), flags=re.S)
    lib = ctypes.CDLL(A.LIB_PATH)
    for name, nargs in (("sgg_warp_affine_u8", 15), ("sgg_resample_f32", 19)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
        assert name in A.SIGNATURES and len(A.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    from sggan_amd import kernels as K
    assert callable(K.warp_affine_u8) and callable(K.resample_f32)
    # argument validation happens before anything touches a device
    p = ctypes.c_void_p(64)
    f = A.lib().sgg_warp_affine_u8
    ok = [p, 1, 8, 16, 3, p, p, p, p, 2, 4, 4, p, 1, None]
    assert all(f(*[bad if i == pos else v for i, v in enumerate(ok)]) == A.EINVAL
               for pos, bad in ((0, None), (4, 2), (9, 17), (10, 0), (12, ctypes.c_void_p(68)), (6, ctypes.c_void_p(12))))
    assert f(*[4096 if i in (10, 11) else (8192 if i in (2, 3) else v) for i, v in enumerate(ok)]) == A.EUNSUPPORTED
    g = A.lib().sgg_resample_f32
    ok = [p, 1, 8, 8, p, p, p, 1, p, p, 1, 1, p, 8 * 8 * 8, 8, 8, 3, A.SGG_F32, None]
    assert all(g(*[bad if i == pos else v for i, v in enumerate(ok)]) == A.EINVAL
               for pos, bad in ((0, None), (16, 5), (7, 9), (10, 0), (17, 7), (13, 8 * 8 * 8 - 8), (13, 8 * 8 * 8 + 4), (0, ctypes.c_void_p(72))))


def test_new_kernels_build_resources(tmp_path):
    """warp.hip and resample.hip recompiled with -Rpass-analysis=kernel-resource-usage: the warp kernel (Cs 3 / 4) and the f32
    resample (bf16 / f32 output) have zero VGPR spills and use no scratch."""
    sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))
    import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    assert "warp.hip" in B.SOURCES and "resample.hip" in B.SOURCES
    for src, kernel, count in (("warp.hip", "warp_affine_u8_kernel", 2), ("resample.hip", "resample_f32_kernel", 2)):
        r = subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, src), "-o", str(tmp_path / (src + ".o")),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        usage, name = {}, None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                usage[name] = {}
                continue
            for key, pat in (("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgprs", r" VGPRs: (\d+)")):
                m = re.search(pat, line)
                if m and name:
                    usage[name][key] = int(m.group(1))
        hits = {k: v for k, v in usage.items() if kernel in k}
        assert len(hits) == count, sorted(usage)
        for k, v in hits.items():
            print(k, v)
            assert v.get("spill") == 0 and v.get("scratch") == 0, (k, v)


def test_command_line_flag():
    from sggan_amd.main import parse_args
    assert parse_args(["--augment"]).augment is True
    assert parse_args([]).augment is False
    assert parse_args([]).use_augmentation is True and parse_args(["--augment"]).use_augmentation is True
    assert parse_args(["--use_augmentation", "x"]).augment is False
