"""generator_unet (reference module.py:125-206) without a GPU: parameter layout, the float64 oracle against an independent torch
float64 statement, the CLI / constructor wiring, the new C-ABI declarations and the register budget of the new kernels."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sggan_amd
from sggan_amd import _abi as A
from sggan_amd.module import generator_param_specs, unet_param_specs
from tests import unet_oracle as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))

N1 = ("sgg_instnorm_fwd_skip", "sgg_instnorm_fwd_skip_partial", "sgg_instnorm_bwd_skip")


def test_unet_param_specs_order_shapes_and_count():
    L = unet_param_specs(64, 3, 3)
    names = [n for n, _ in L]
    exp = []
    for i in range(1, 9):
        exp += [f"e{i}_w", f"e{i}_b", f"e{i}_g", f"e{i}_beta"]
    for i in range(1, 8):
        exp += [f"d{i}_w", f"d{i}_b", f"d{i}_g", f"d{i}_beta"]
    exp += ["d8_w", "d8_b"]
    assert names == exp
    S = dict(L)
    assert [S[f"e{i}_w"] for i in range(1, 9)] == [(3, 3, 3, 64), (3, 3, 64, 128), (3, 3, 128, 256), (3, 3, 256, 512)] + [(3, 3, 512, 512)] * 4
    # Conv2DTranspose kernels are (kh, kw, out, in)
    assert [S[f"d{i}_w"] for i in range(1, 9)] == [(3, 3, 512, 512)] * 4 + [(3, 3, 256, 512), (3, 3, 128, 256), (3, 3, 64, 128), (3, 3, 3, 64)]
    assert S["d8_b"] == (3,) and S["d5_g"] == (256,)
    assert sum(int(np.prod(s)) for _, s in L) == 21_990_915
    assert L == [(n, tuple(s)) for n, s in U.unet_param_shapes(64, 3, 3)]       # the oracle's independent statement
    assert sum(int(np.prod(s)) for _, s in generator_param_specs()) != 21_990_915


def test_unet_oracle_matches_torch_float64_restatement():
    """The NumPy tape oracle and the torch autograd statement agree on the output and on every gradient (parameters and input)."""
    rng = np.random.default_rng(5)
    shapes = U.unet_param_shapes(4, 3, 3)
    from oracle import sggan_oracle as O
    PG = O.init_params(shapes, rng, perturb=0.1)
    x = rng.uniform(0, 1, (2, 8, 12, 3))
    dy = rng.standard_normal((2, 8, 12, 3))
    y0, g0, dx0 = U.generator_forward_backward(PG, x, dy)
    y1, g1, dx1 = U.torch_forward_backward(PG, x, dy)
    scale = lambda a: max(np.abs(a).max(), 1e-30)
    assert np.abs(y0 - y1).max() < 1e-10
    assert np.abs(dx0 - dx1).max() < 1e-10 * max(1.0, scale(dx1))
    for k in g1:
        assert np.abs(g0[k] - g1[k]).max() < 1e-10 * max(1.0, scale(g1[k])), k
    # the skip adds are live: the gradient reaches every encoder layer through more than the conv chain
    assert all(np.abs(g1[f"e{i}_w"]).max() > 0 for i in range(1, 9))


def test_cli_generator_flag_and_unsupported_combinations():
    from sggan_amd.main import parse_args
    assert parse_args(["--generator", "unet"]).use_resnet is False
    assert parse_args([]).use_resnet is True                          # today's default stays the ResNet
    assert parse_args(["--generator", "resnet"]).use_resnet is True
    with pytest.raises(SystemExit):
        parse_args(["--generator", "pix2pix"])
    # the checks that refuse a configuration run before any network (and so any device) is touched
    with pytest.raises(NotImplementedError, match="pix2pix"):
        sggan_amd.sggan(sggan_amd.default_args(use_pix2pix=True, device="cpu"))
    with pytest.raises(NotImplementedError, match="cycle"):
        sggan_amd.sggan(sggan_amd.default_args(use_resnet=False, cycle=True, device="cpu"))


def test_skip_norm_exports_declared_in_header_and_abi():
    src = open(os.path.join(ROOT, "include", "sggan.h")).read()
    for name in N1:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in A.SIGNATURES, name
    assert len(A.SIGNATURES["sgg_instnorm_bwd_skip"][1]) == 21


def test_skip_norm_kernels_do_not_spill(tmp_path):
    import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, "norm.hip"), "-o", str(tmp_path / "norm.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            usage[name]["spill"] = int(m.group(1))
    for frag in ("in_apply_skip_kernelI", "in_skip_bwd_partial_kernelI"):
        hits = {k: v for k, v in usage.items() if frag in k}
        assert len(hits) == 2, (frag, list(hits))                     # bf16 and f32
        for k, v in hits.items():
            assert v.get("spill") == 0, (k, v)
