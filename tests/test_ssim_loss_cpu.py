"""The structural-similarity training loss without a GPU (--ssim_lambda): the closed-form gradient of
tests/ssim_loss_oracle.py against torch float64 autograd, the exact zero of identical operands, the C-ABI declarations, the
refusals sgg_ssim_loss answers from the host in their documented order, the resources of csrc/ssimloss.hip, and the flags."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from sggan_amd import _abi as A
from tests import ssim_loss_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))

EXPORTS = {"sgg_ssim_loss_workspace": 4, "sgg_ssim_loss": 17}
SL_TH, SL_TW = 16, 32                                   # csrc/ssimloss.hip; tests/test_gpu_ssim_loss.py repeats them


def _grid(rng, shape):
    return rng.integers(0, 65, shape).astype(np.float64) / 64.0


# ---- the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(11, 11), (12, 27), (27, 43)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("data_range", [1.0, 2.0])
def test_closed_form_gradient_is_float64_autograd(hw, data_range):
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    t, x = _grid(rng, (2,) + hw + (3,)), _grid(rng, (2,) + hw + (3,))
    xt = torch.from_numpy(x).requires_grad_(True)
    L = SO.loss_torch(torch.from_numpy(t), xt, data_range)
    L.backward()
    g = SO.grad(t, x, data_range)
    assert abs(L.item() - SO.loss(t, x, data_range)) <= 1e-15
    err = np.abs(g - xt.grad.numpy()).max() / np.abs(g).max()
    print(f"closed form vs autograd at {hw}: {err:.2e} of max|g| = {np.abs(g).max():.3e}")
    assert err <= 1e-12
    M = SO.magnitude(t, x, data_range)
    assert M.shape == g.shape and np.all(M >= np.abs(g) * (1 - 1e-12))


def test_identical_operands_give_exactly_zero_loss_and_one_everywhere():
    rng = np.random.default_rng(5)
    x = _grid(rng, (2, 19, 23, 3))
    x[0, :, :12] = 0.25                                   # a piecewise-constant stretch: E[xx] - ux^2 cancels to rounding noise
    assert np.all(SO.ssim_map(x, x) == 1.0) and SO.loss(x, x) == 0.0
    assert SO.loss(x, x, data_range=255.0) == 0.0


def test_window_and_adjoint_are_consistent():
    w = SO.window()
    assert w.shape == (11,) and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1]) and w.argmax() == 5
    rng = np.random.default_rng(6)
    a, c = rng.standard_normal((1, 14, 17, 2)), rng.standard_normal((1, 4, 7, 2))
    assert abs((SO._filt(a) * c).sum() - (a * SO._adj(c)).sum()) < 1e-12          # <G a, c> == <a, G^T c>
    one = np.ones((1, 1, 1, 1))
    assert np.allclose(SO._adj(one)[0, :, :, 0], np.outer(w, w), rtol=0, atol=1e-17)   # an 11x11 image: one window feeds each pixel once


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_exports_declared_in_header_abi_and_library():
    import build as B
    assert "ssimloss.hip" in B.SOURCES
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sggan.h")).read(), flags=re.S)
    assert os.path.exists(A.LIB_PATH), "run `python __graft_entry__.py build` first"
    L = ctypes.CDLL(A.LIB_PATH)
    for name, nargs in EXPORTS.items():
        decl = re.search(r"(?:int|size_t)\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in A.SIGNATURES and len(A.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name), f"{name} not exported by libsggan.so"
    assert A.SIGNATURES["sgg_ssim_loss_workspace"][0] is ctypes.c_size_t


def test_host_side_refusals_in_their_documented_order():
    """Everything sgg_ssim_loss refuses before it launches, answered from the host with pointers that are never dereferenced.
    Order: SGG_EINVAL reasons, then SGG_EUNSUPPORTED, then SGG_EWORKSPACE -- a call wrong in two ways gives the earlier answer."""
    L = A.lib()
    GB = 1 << 32                                                                         # far apart: no claimed extent overlaps
    t, x, dx, loss, ws = (ctypes.c_void_p(a) for a in (1 * GB, 2 * GB, 3 * GB, 4 * GB, 5 * GB))
    need = L.sgg_ssim_loss_workspace(2, 64, 48, 3)
    tiles = ((64 - 10 + SL_TH - 1) // SL_TH) * ((48 - 10 + SL_TW - 1) // SL_TW)
    assert need == 8 * (2 * 3 * 3 * 54 * 38 + 2 * tiles)
    assert L.sgg_ssim_loss_workspace(1, 11, 11, 1) == 8 * (3 + 1)
    assert L.sgg_ssim_loss_workspace(8, 512, 256, 3) == 8 * (8 * 3 * 3 * 502 * 246 + 8 * 32 * 8)      # 71.1 MB

    def call(t=t, x=x, N=2, H=64, W=48, Cr=3, Cp=8, dr=1.0, loss=loss, dx=dx, dtype=A.SGG_BF16, ws=ws, nbytes=need):
        return L.sgg_ssim_loss(t, x, N, H, W, Cr, Cp, dr, 1.0, 1.0, loss, dx, 0, dtype, ws, nbytes, None)
    # SGG_EINVAL
    assert call(t=None) == A.EINVAL and call(x=None) == A.EINVAL and call(loss=None) == A.EINVAL and call(ws=None) == A.EINVAL
    assert call(t=ctypes.c_void_p(1 * GB + 8)) == A.EINVAL and call(x=ctypes.c_void_p(2 * GB + 2)) == A.EINVAL
    assert call(dx=ctypes.c_void_p(3 * GB + 4)) == A.EINVAL and call(ws=ctypes.c_void_p(5 * GB + 8)) == A.EINVAL
    assert call(dx=x) == A.EINVAL and call(dx=t) == A.EINVAL
    assert call(dx=ctypes.c_void_p(2 * GB + 16)) == A.EINVAL                          # inside x
    assert call(N=0) == A.EINVAL and call(N=-1) == A.EINVAL
    assert call(Cr=0) == A.EINVAL and call(Cr=9) == A.EINVAL
    assert call(dtype=A.SGG_U8) == A.EINVAL and call(dtype=-1) == A.EINVAL
    assert call(dr=0.0) == A.EINVAL and call(dr=-1.0) == A.EINVAL and call(dr=float("inf")) == A.EINVAL and call(dr=float("nan")) == A.EINVAL
    # ... before SGG_EUNSUPPORTED and SGG_EWORKSPACE
    assert call(x=None, H=10) == A.EINVAL and call(dr=0.0, H=10, nbytes=0) == A.EINVAL and call(dx=x, nbytes=0) == A.EINVAL
    # SGG_EUNSUPPORTED, where the workspace query says 0
    assert call(H=10) == A.EUNSUPPORTED and call(W=10) == A.EUNSUPPORTED and call(H=2048, W=2049) == A.EUNSUPPORTED
    assert call(Cp=16) == A.EUNSUPPORTED and call(H=1 << 16, W=1 << 16, dx=None) == A.EUNSUPPORTED
    assert call(H=10, nbytes=0) == A.EUNSUPPORTED                                       # ... before SGG_EWORKSPACE
    for shape in ((1, 10, 48, 3), (1, 64, 10, 3), (1, 2048, 2049, 3), (0, 64, 48, 3)):
        assert L.sgg_ssim_loss_workspace(*shape) == 0
    # SGG_EWORKSPACE
    assert call(nbytes=need - 1) == A.EWORKSPACE and call(nbytes=0) == A.EWORKSPACE and call(dx=None, nbytes=need - 1) == A.EWORKSPACE
    assert call(N=3) == A.EWORKSPACE                                                     # one more image needs more


def test_ssimloss_kernels_use_no_scratch_do_not_spill_and_fit_64k_of_lds(tmp_path):
    import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, "ssimloss.hip"), "-o", str(tmp_path / "ssimloss.o"),
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
    # three launches at most: forward and adjoint per storage type, and the fold
    assert sorted(sum(w in k for k in usage) for w in ("ssim_loss_fwd_kernel", "ssim_loss_bwd_kernel", "ssim_loss_fold_kernel")) == [1, 2, 2]
    assert len(usage) == 5, sorted(usage)
    for k, v in usage.items():
        assert (v["vspill"], v["sspill"], v["scratch"]) == (0, 0, 0), (k, v)
        assert v["lds"] <= 65536, (k, v)                                                 # two blocks share a CU


def test_tile_constants_of_the_source_are_the_ones_the_tests_use():
    src = open(os.path.join(ROOT, "sg-gan-tf2_amd", "csrc", "ssimloss.hip")).read()
    th, tw = re.search(r"\bSL_TH\s*=\s*(\d+)", src), re.search(r"\bSL_TW\s*=\s*(\d+)", src)
    assert th and tw and (int(th.group(1)), int(tw.group(1))) == (SL_TH, SL_TW)
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_ssim_loss.py")).read()
    m = re.search(r"^SL_TH, SL_TW = (\d+), (\d+)", gpu, flags=re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == (SL_TH, SL_TW)


# ---- the flags -----------------------------------------------------------------------------------------------------------
def test_flags_are_absent_unless_given_and_parse_when_given():
    from sggan_amd.main import build_parser, parse_args
    bare = parse_args([])
    assert "ssim_lambda" not in vars(bare) and "ssim_data_range" not in vars(bare)
    a = parse_args(["--ssim_lambda", "2.5", "--ssim_data_range", "2"])
    assert a.ssim_lambda == 2.5 and a.ssim_data_range == 2.0
    assert vars(a).keys() - vars(bare).keys() == {"ssim_lambda", "ssim_data_range"}
    assert all(getattr(a, k) == v for k, v in vars(bare).items())
    assert not hasattr(parse_args(["--ssim_lambda", "1"]), "ssim_data_range")
    text = build_parser().format_help()
    assert "--ssim_lambda" in text and "--ssim_data_range" in text
