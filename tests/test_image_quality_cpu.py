"""Paired image-quality scores without a GPU: the oracle's own facts on cases worked by hand, its window against
scipy's Gaussian filter, the C-ABI declarations, the refusals the library answers from the host, the resources of
csrc/imgqual.hip, the tile constants the GPU tests repeat, and the flag."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from sggan_amd import _abi as A
from tests import image_quality_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))

EXPORTS = {"sgg_image_quality_workspace": 3, "sgg_image_quality": 13}
IQ_TH, IQ_TW = 16, 32                                   # csrc/imgqual.hip; tests/test_gpu_image_quality.py repeats them


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def test_oracle_quantises_like_inverse_transform_and_clamps():
    x = np.array([[[[-1.0, 1.0, 0.0], [-1.0001, 1.0001, np.nan], [np.inf, -np.inf, 0.999], [-0.999, 0.5, -0.5]]]], dtype=np.float32)
    assert O.quantise(x)[0, 0].tolist() == [[0, 255, 127], [0, 255, 0], [255, 0, 254], [0, 191, 63]]
    from sggan_amd.utils import inverse_transform
    inside = np.linspace(-1, 1, 4099, dtype=np.float32).reshape(1, 1, -1, 1).repeat(3, axis=3)
    assert np.array_equal(O.quantise(inside), inverse_transform(inside).astype(np.int64))
    u8 = np.arange(24, dtype=np.uint8).reshape(1, 2, 3, 4)
    assert np.array_equal(O.quantise(u8), u8[..., :3].astype(np.int64))                   # the fourth channel is not used


def test_oracle_window_is_the_normalised_gaussian():
    w = O.window()
    assert w.shape == (11,) and abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w[::-1])
    assert abs(w[5] / w[4] - np.exp(1.0 / 4.5)) < 1e-15 and abs(w[5] / w[0] - np.exp(25.0 / 4.5)) < 1e-12


def test_identical_images_give_ssim_exactly_one_and_zero_sums():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (2, 13, 17, 3)).astype(np.uint8)
    s = O.sums(a, a.copy())
    assert np.array_equal(s, np.array([[0.0, 0.0, 3 * 3 * 7]] * 2))
    assert np.array_equal(O.ssim_map(O.quantise(a), O.quantise(a)), np.ones((2, 3, 7, 3)))
    sc = O.scores(a, a)
    assert np.array_equal(sc["SSIM"], [1.0, 1.0]) and np.array_equal(sc["MAE"], [0.0, 0.0]) and np.isinf(sc["PSNR"]).all()


@pytest.mark.parametrize("c1,c2", [(10, 200), (255, 0), (128, 127), (37, 91), (255, 254), (1, 255), (0, 0)])
def test_two_constant_images_give_the_closed_form(c1, c2):
    a, b = np.full((1, 13, 14, 3), c1, dtype=np.uint8), np.full((1, 13, 14, 3), c2, dtype=np.uint8)
    want = (2.0 * c1 * c2 + O.C1) / (c1 * c1 + c2 * c2 + O.C1)
    S = O.ssim_map(O.quantise(a), O.quantise(b))
    assert S.shape == (1, 3, 4, 3) and np.abs(S - want).max() <= 1e-15
    sc = O.scores(a, b)
    assert sc["MAE"][0] == abs(c1 - c2) and sc["MSE"][0] == (c1 - c2) ** 2


def test_border_pixels_of_an_11x11_image_reach_ssim_only_through_the_one_window():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (1, 11, 11, 3)).astype(np.uint8)
    b = rng.integers(0, 256, (1, 11, 11, 3)).astype(np.uint8)
    b2 = b.copy()
    b2[0, 0, 0] = 255 - b2[0, 0, 0]                       # a corner and an edge pixel: within 5 of the border
    b2[0, 10, 4, 1] ^= 0x80
    assert not np.array_equal(b, b2) and np.array_equal(b[0, 1:10, 1:], b2[0, 1:10, 1:])
    s, s2 = O.sums(a, b), O.sums(a, b2)
    d = np.abs(a.astype(np.int64) - b2)
    assert s2[0, 0] == d.sum() and s2[0, 0] != s[0, 0] and s2[0, 1] == (d * d).sum()
    # the hand sum: ONE window per channel, the plain weighted moments over all 121 pixels
    w2 = np.outer(O.window(), O.window())
    hand = 0.0
    for c in range(3):
        x, y = a[0, :, :, c].astype(np.float64), b2[0, :, :, c].astype(np.float64)
        ux, uy = (w2 * x).sum(), (w2 * y).sum()
        vx, vy, vxy = (w2 * x * x).sum() - ux * ux, (w2 * y * y).sum() - uy * uy, (w2 * x * y).sum() - ux * uy
        hand += (2 * ux * uy + O.C1) * (2 * vxy + O.C2) / ((ux * ux + uy * uy + O.C1) * (vx + vy + O.C2))
    assert O.ssim_map(O.quantise(a), O.quantise(b2)).shape == (1, 1, 1, 3)
    assert abs(s2[0, 2] - hand) <= 1e-12 and abs(s2[0, 2] - s[0, 2]) > 1e-6          # changed, and only through that window
    assert O.counts(11, 11) == (363, 3)


def test_oracle_ssim_equals_scipy_gaussian_filter_cropped_by_five():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (2, 23, 31, 3)).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    got = O.scores(a, b)["SSIM"]
    for n in range(2):
        per_channel = []
        for c in range(3):
            x, y = a[n, :, :, c].astype(np.float64), b[n, :, :, c].astype(np.float64)
            f = lambda v: ndi.gaussian_filter(v, sigma=1.5, truncate=3.5)            # radius int(3.5 * 1.5 + 0.5) = 5
            ux, uy = f(x), f(y)
            vx, vy, vxy = f(x * x) - ux * ux, f(y * y) - uy * uy, f(x * y) - ux * uy
            S = (2 * ux * uy + O.C1) * (2 * vxy + O.C2) / ((ux * ux + uy * uy + O.C1) * (vx + vy + O.C2))
            per_channel.append(S[5:-5, 5:-5].mean())
        assert abs(got[n] - np.mean(per_channel)) <= 1e-12, (n, got[n], np.mean(per_channel))


def test_pooled_scores_use_the_finite_psnr_bound_for_identical_images():
    rows = np.array([[0.0, 0.0, 3 * 2 * 3], [0.0, 0.0, 3 * 2 * 3]])
    p = O.pooled(rows, 12, 13)
    assert p["MAE"] == 0.0 and p["SSIM"] == 1.0 and p["PSNR"] == 10.0 * np.log10(255.0 ** 2 * (2 * 3 * 12 * 13)) and np.isfinite(p["PSNR"])
    rows = np.array([[30.0, 100.0, 9.0], [10.0, 20.0, 18.0]])
    p = O.pooled(rows, 12, 13)
    assert p["MAE"] == 40.0 / 936 and p["PSNR"] == 10.0 * np.log10(255.0 ** 2 / (120.0 / 936)) and p["SSIM"] == (0.5 + 1.0) / 2


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_exports_declared_in_header_abi_and_library():
    import build as B
    assert "imgqual.hip" in B.SOURCES
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sggan.h")).read(), flags=re.S)
    assert os.path.exists(A.LIB_PATH), "run `python __graft_entry__.py build` first"
    L = ctypes.CDLL(A.LIB_PATH)
    for name, nargs in EXPORTS.items():
        decl = re.search(r"(?:int|size_t)\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in A.SIGNATURES and len(A.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name), f"{name} not exported by libsggan.so"
    assert A.SIGNATURES["sgg_image_quality_workspace"][0] is ctypes.c_size_t


def test_host_side_argument_checks_without_gpu():
    """Everything sgg_image_quality refuses before it launches: answered from the host, no device needed."""
    L = A.lib()
    x = ctypes.c_void_p(4096)                                                        # never dereferenced by a refused call
    need = L.sgg_image_quality_workspace(2, 64, 48)
    tiles = ((64 - 10 + IQ_TH - 1) // IQ_TH) * ((48 - 10 + IQ_TW - 1) // IQ_TW)
    assert need == 2 * tiles * 24 and L.sgg_image_quality_workspace(1, 11, 11) == 24

    def call(a=x, ka=A.SGG_BF16, ca=8, b=x, kb=A.SGG_U8, cb=3, N=2, H=64, W=48, out=x, ws=x, nbytes=need):
        return L.sgg_image_quality(a, ka, ca, b, kb, cb, N, H, W, out, ws, nbytes, None)
    assert call(a=None) == A.EINVAL and call(b=None) == A.EINVAL and call(out=None) == A.EINVAL and call(ws=None) == A.EINVAL
    assert call(ka=3) == A.EINVAL and call(kb=-1) == A.EINVAL
    assert call(ca=2) == A.EINVAL and call(ka=A.SGG_F32, ca=2) == A.EINVAL and call(cb=2) == A.EINVAL and call(cb=5) == A.EINVAL
    assert call(ka=A.SGG_U8, ca=8) == A.EINVAL and call(kb=A.SGG_F32, cb=1) == A.EINVAL
    assert call(N=0) == A.EINVAL and call(N=-1) == A.EINVAL
    assert call(H=10) == A.EUNSUPPORTED and call(W=10) == A.EUNSUPPORTED and call(H=2048, W=2049) == A.EUNSUPPORTED
    assert call(H=1 << 16, W=1 << 16) == A.EUNSUPPORTED                                # H * W past 32 bits
    assert call(nbytes=need - 1) == A.EWORKSPACE and call(nbytes=0) == A.EWORKSPACE
    assert call(H=2048, W=2048, N=1, nbytes=need) == A.EWORKSPACE                      # the largest supported shape needs more
    for shape in ((0, 64, 48), (1, 10, 48), (1, 64, 10), (1, 2048, 2049)):
        assert L.sgg_image_quality_workspace(*shape) == 0
    assert L.sgg_image_quality_workspace(1, 2048, 2048) == 24 * 128 * 64


def test_imgqual_kernels_use_no_scratch_do_not_spill_and_fit_64k_of_lds(tmp_path):
    import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    assert "imgqual.hip" in B.SOURCES
    r = subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, "imgqual.hip"), "-o", str(tmp_path / "imgqual.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        for key, pat in (("vspill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                usage[name][key] = int(m.group(1))
    assert sum("image_quality_kernel" in k for k in usage) == 1 and sum("image_quality_fold_kernel" in k for k in usage) == 1
    assert len(usage) == 2, sorted(usage)                                              # at most two launches: two kernels
    for k, v in usage.items():
        assert (v["vspill"], v["sspill"], v["scratch"]) == (0, 0, 0), (k, v)
        assert v["lds"] <= 65536, (k, v)


def test_tile_constants_of_the_source_are_the_ones_the_tests_use():
    src = open(os.path.join(ROOT, "sg-gan-tf2_amd", "csrc", "imgqual.hip")).read()
    th, tw = re.search(r"\bIQ_TH\s*=\s*(\d+)", src), re.search(r"\bIQ_TW\s*=\s*(\d+)", src)
    assert th and tw and (int(th.group(1)), int(tw.group(1))) == (IQ_TH, IQ_TW)
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_image_quality.py")).read()
    m = re.search(r"^IQ_TH, IQ_TW = (\d+), (\d+)", gpu, flags=re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == (IQ_TH, IQ_TW)


# ---- the flag ------------------------------------------------------------------------------------------------------------
def test_flag_is_absent_unless_given_and_parses_when_given():
    from sggan_amd.main import parse_args
    bare = parse_args([])
    assert not hasattr(bare, "image_scores")
    a = parse_args(["--image_scores"])
    assert a.image_scores is True
    assert vars(a).keys() - vars(bare).keys() == {"image_scores"}
    assert all(getattr(a, k) == v for k, v in vars(bare).items())
