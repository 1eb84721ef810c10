"""Cycle mode with the U-Net generators, without a GPU: the float64 cycle-step oracle (tests/unet_cycle_oracle.py) against an
independent torch autograd statement, the C-ABI declarations of the lockstep skip norm, and its kernels' register budget."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import sggan_oracle as O
from sggan_amd import _abi as A
from tests import unet_cycle_oracle as UC
from tests import unet_oracle as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))

# export -> number of arguments (the single forms + gamma2, beta2, nsplit [+ dgamma2, dbeta2])
PAIR = {"sgg_instnorm_fwd_skip_pair": 19, "sgg_instnorm_fwd_skip_partial_pair": 19, "sgg_instnorm_bwd_skip_pair": 26}


@pytest.mark.parametrize("use_lsgan", [True, False], ids=["lsgan", "sce"])
def test_unet_cycle_oracle_matches_torch_float64_autograd(use_lsgan):
    """1x128x128, ngf 4, ndf 4: both losses and every gradient tensor of the four networks agree to 1e-9 of the tensor's largest
    entry (two float64 evaluations of the same function in different summation orders: ~1e-13 is expected)."""
    rng = np.random.default_rng(41)
    gs, ds = U.unet_param_shapes(4, 3, 3), O.discriminator_param_shapes(df_dim=4)
    P = {n: O.init_params(sh, rng, 0.1) for n, sh in (("Gab", gs), ("Gba", gs), ("Da", ds), ("Db", ds))}
    N, H, W = 1, 128, 128
    real_A, real_B = rng.uniform(0, 1, (N, H, W, 3)), rng.uniform(0, 1, (N, H, W, 3))
    pal = rng.integers(0, 256, (8, 3)) / 255.0
    blocks = lambda: pal[np.repeat(np.repeat(rng.integers(0, 8, (N, H // 32, W // 32)), 32, 1), 32, 2)]
    seg_A, seg_B = blocks(), blocks()
    mk = lambda: np.stack([O.one_hot(i, 34) for i in rng.integers(0, 34, (N, 4, 4))]).astype(np.float64)
    mask_A, mask_B = mk(), mk()
    r = UC.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], real_A, real_B, seg_A, seg_B, mask_A, mask_B, use_lsgan=use_lsgan)
    t = UC.torch_cycle_step(P, real_A, real_B, seg_A, seg_B, mask_A, mask_B, use_lsgan=use_lsgan)
    assert abs(r["g_loss"] - t["g_loss"]) < 1e-9 * abs(t["g_loss"]) and abs(r["d_loss"] - t["d_loss"]) < 1e-9 * abs(t["d_loss"])
    for k in ("fake_A", "fake_B", "cyc_A", "cyc_B"):
        assert np.abs(r[k] - t[k]).max() < 1e-9, k
    worst, live = 0.0, 0
    for n in UC.NETS:
        for k, e in t["grads"][n].items():
            got = r["grads"][n][k]
            if np.abs(e).max() < 1e-12:                   # a bias in front of an instance norm: identically zero in both
                assert np.abs(got).max() < 1e-12, (n, k)
                continue
            err = np.abs(got - e).max() / np.abs(e).max()
            worst, live = max(worst, err), live + 1
            assert err < 1e-9, (n, k, err)
    print(f"oracle vs autograd [{'lsgan' if use_lsgan else 'sce'}]: {live} gradient tensors, worst relative error {worst:.1e}")
    # every generator tensor but the 15 biases in front of a norm is reached (16 kernels, 15 gamma / beta pairs, d8's bias); at
    # 128x128 the discriminators' h33 map is 1x1, where the instance norm returns beta whatever its input: h33_beta, h4_w, h4_b
    assert live == 2 * (16 + 2 * 15 + 1) + 2 * 3


def test_pair_skip_norm_exports_in_header_abi_and_library():
    src = open(os.path.join(ROOT, "include", "sggan.h")).read()
    import build as B
    lib = ctypes.CDLL(B.build_lib())
    for name, nargs in PAIR.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, len(m.group(1).split(",")))
        assert name in A.SIGNATURES and len(A.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None
    # the pair forms take the single forms' arguments plus the second parameter set
    assert len(A.SIGNATURES["sgg_instnorm_fwd_skip_pair"][1]) == len(A.SIGNATURES["sgg_instnorm_fwd_skip"][1]) + 3
    assert len(A.SIGNATURES["sgg_instnorm_fwd_skip_partial_pair"][1]) == len(A.SIGNATURES["sgg_instnorm_fwd_skip_partial"][1]) + 3
    assert len(A.SIGNATURES["sgg_instnorm_bwd_skip_pair"][1]) == len(A.SIGNATURES["sgg_instnorm_bwd_skip"][1]) + 5


def test_pair_skip_norm_kernels_do_not_spill_and_use_no_scratch(tmp_path):
    """The kernels the lockstep skip norm launches -- in_apply_skip_kernel (now with the split argument), the backward's dz /
    statistics pass and the shared apply kernel in_apply_kernel -- build without VGPR spills and without scratch."""
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
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                usage[name][key] = int(m.group(1))
    for frag, count in (("in_apply_skip_kernelI", 2), ("in_skip_bwd_partial_kernelI", 2), ("in_apply_kernelI", 5)):
        hits = {k: v for k, v in usage.items() if frag in k}
        assert len(hits) == count, (frag, list(hits))
        for k, v in hits.items():
            print(f"{k}: {v['vgprs']} VGPRs, {v['spill']} spilled, {v['scratch']} bytes scratch")
            assert v["spill"] == 0 and v["scratch"] == 0, (k, v)
    # the split is an argument of the skip apply kernel (one kernel serves the single and the lockstep entry points)
    assert all("InSplit" in k or k.endswith("7InSplit") for k in usage if "in_apply_skip_kernelI" in k)


@pytest.mark.parametrize("kw", [dict(), dict(cycle=True), dict(use_resnet=False), dict(use_resnet=False, cycle=True)],
                         ids=["resnet", "resnet_cycle", "unet", "unet_cycle"])
def test_constructor_refuses_a_host_device_for_every_configuration_before_building_networks(kw):
    """No configuration has a host implementation: sggan() says so by name -- mode and generator -- before a network is built
    (module._Net would raise for the first network it builds; the step-level message names what was asked for).  The U-Net
    cycle combination is refused for the device only: nothing else stands in its way."""
    import sggan_amd
    with pytest.raises(NotImplementedError, match=r"cycle=%s, generator=%s\) on device 'cpu'.*HIP path only"
                       % (bool(kw.get("cycle")), "resnet" if kw.get("use_resnet", True) else "unet")):
        sggan_amd.sggan(sggan_amd.default_args(device="cpu", **kw))
