"""Training-mode dropout of the U-Net decoder without a GPU: the oracle's Philox against the scalar one, the
mask's statistics and independence, the threshold arithmetic, the oracle's own gradients against central differences, the
library's argument checks (answered before any launch), the flag and the constructor, and the kernels' resource usage."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import sggan_amd
from sggan_amd import _abi as A
from sggan_amd import kernels as K
from tests import diffaug_oracle as DA
from tests import dropout_oracle as DO
from tests.kernel_resources import kernel_resource_usage, the_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [(0, 19, 0), (1, 19, 0), (7, 21, 5), (2 ** 33 + 1, 19, 2)]          # (t, seed, stream)


def test_vectorised_philox_equals_the_scalar_statement():
    rng = np.random.default_rng(3)
    e = np.concatenate([[0, 1, 2 ** 32 - 1], rng.integers(0, 2 ** 32, 13)]).astype(np.uint64)
    for t, seed, stream in KEYS:
        c0, c1, g, key = t & 0xFFFFFFFF, t >> 32, 5 + stream, (seed, 1 + stream)
        got = np.stack(DO.philox4x32_10(c0, c1, g, e, key), -1)
        want = np.array([DA.philox4x32_10((c0, c1, g, int(v)), key) for v in e], np.uint32)
        assert np.array_equal(got, want)
    # the draws: lane j of vector e is half j & 1 of word j >> 1
    d = DO.draws(7, 21, 5, 3, 4)
    for e_ in range(4):
        r = DA.philox4x32_10((7, 0, 3, e_), (21, 6))
        assert [int(v) for v in d[8 * e_:8 * e_ + 8]] == [(r[j >> 1] >> (16 * (j & 1))) & 0xFFFF for j in range(8)]


@pytest.mark.parametrize("rate", [0.5, 0.2, 0.9])
@pytest.mark.parametrize("key", KEYS, ids=[f"t{t}-s{s}-k{k}" for t, s, k in KEYS])
def test_kept_fraction_is_the_thresholds(key, rate):
    """The kept fraction over (2, 16*16*64) lies within 4 sigma of 1 - threshold / 65536 (measured: all twelve within 1.6)."""
    t, seed, stream = key
    n, elems = 2, 16 * 16 * 64
    m = DO.keep_mask(t, seed, stream, 0, n, elems, rate)
    p = 1.0 - DO.threshold(rate) / 65536.0
    sigma = math.sqrt(p * (1 - p) / (n * elems))
    dev = abs(m.mean() - p) / sigma
    print(f"key {key} rate {rate}: kept {m.mean():.5f}, expected {p:.5f}, {dev:.2f} sigma")
    assert m.shape == (n, elems) and dev < 4.0


@pytest.mark.parametrize("what", ["t", "stream_id", "sample"])
def test_masks_of_different_keys_are_independent(what):
    """Two rate-0.5 masks of 2^17 draws that differ only in t, only in stream_id or only in the sample agree on a fraction
    within 4 sigma of 0.5 (measured: all three within 1.3)."""
    n = 2 ** 17
    a = DO.keep_mask(3, 19, 1, 0, 1, n, 0.5)
    b = {"t": lambda: DO.keep_mask(4, 19, 1, 0, 1, n, 0.5), "stream_id": lambda: DO.keep_mask(3, 19, 2, 0, 1, n, 0.5),
         "sample": lambda: DO.keep_mask(3, 19, 1, 1, 1, n, 0.5)}[what]()
    agree = float((a == b).mean())
    dev = abs(agree - 0.5) / (0.5 / math.sqrt(n))
    print(f"differ in {what}: agree on {agree:.5f}, {dev:.2f} sigma")
    assert dev < 4.0
    # ... and a row of a two-row mask is the one-row mask of that sample
    assert np.array_equal(DO.keep_mask(3, 19, 1, 0, 2, 4096, 0.5)[1], DO.keep_mask(3, 19, 1, 1, 1, 4096, 0.5)[0])


def test_threshold_arithmetic():
    assert DO.threshold(0.0) == 0 and DO.threshold(0.5) == 32768 and DO.threshold(0.2) == 13107 and DO.threshold(0.99999999) == 65535
    assert [K.dropout_threshold(r) for r in (0.0, 0.2, 0.5, 0.9)] == [DO.threshold(r) for r in (0.0, 0.2, 0.5, 0.9)]
    assert DO.scale(32768) == np.float32(2.0) and DO.scale(0) == np.float32(1.0)
    x = np.array([1.5, -0.0, 3e-39, -7.25, np.inf, 1.0, 2.0, 3.0], np.float32)
    keep = DO.keep_mask(0, 19, 0, 0, 1, 8, 0.0)
    assert keep.all() and np.array_equal(DO.apply(x, keep, 0.0).view(np.uint32), x.view(np.uint32))       # rate 0: the identity
    m = np.array([1, 0, 1, 1, 0, 1, 0, 1], bool)
    got = DO.apply(x, m, 0.5)
    assert np.array_equal(got, np.where(m, 2 * x, 0)) and not np.signbit(got[1])                          # dropped: +0
    xb = torch.tensor([1.0, 1.0078125, 3.0, -1.0078125, 0.5, 0.25, 2.0, 4.0]).numpy()                     # bf16 values
    gb = DO.apply(xb, np.ones(8, bool), 0.2, bf16=True)
    want = torch.from_numpy((xb * (np.float32(65536) / np.float32(65536 - 13107))).astype(np.float32)).to(torch.bfloat16).float().numpy()
    assert np.array_equal(gb, want) and np.array_equal(gb, torch.from_numpy(gb).to(torch.bfloat16).float().numpy())
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            K.dropout_threshold(bad)


def _layer_case(masked):
    rng = np.random.default_rng(5)
    N, H, W, Ci, Co = 1, 6, 6, 8, 8
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    h, dy = t64(rng.standard_normal((N, Ci, H, W))), t64(rng.standard_normal((N, Co, H, W)))
    w, b = t64(rng.standard_normal((3, 3, Co, Ci)) * 0.2), t64(rng.standard_normal(Co) * 0.3)
    gamma, beta = t64(1 + 0.2 * rng.standard_normal(Co)), t64(0.2 * rng.standard_normal(Co))
    mask = torch.from_numpy(DO.layer_mask(2, 19, 1, 0, N, H, W, Co, 0.5).astype(np.float64)).permute(0, 3, 1, 2) if masked else None
    loss = lambda bb: float((DO.masked_deconv_norm(h, w, bb, gamma, beta, mask, 2.0) * dy).sum())
    br = b.clone().requires_grad_(True)
    (DO.masked_deconv_norm(h, w, br, gamma, beta, mask, 2.0) * dy).sum().backward()
    return b, br.grad.numpy(), loss


def test_oracle_bias_gradient_of_a_dropout_layer():
    """deconv -> mask * scale -> IN: the oracle's bias gradient equals central differences, is non-zero with a mask (the norm
    no longer cancels the bias) and below 1e-9 without one."""
    b, gb, loss = _layer_case(True)
    eps = 1e-6
    num = np.array([(loss(b + eps * torch.eye(len(b), dtype=torch.float64)[k]) - loss(b - eps * torch.eye(len(b), dtype=torch.float64)[k])) / (2 * eps)
                    for k in range(len(b))])
    assert np.abs(gb).min() > 1e-3 and np.abs(gb - num).max() < 1e-6 * np.abs(gb).max()
    _, g0, _ = _layer_case(False)
    assert np.abs(g0).max() < 1e-9


def test_masked_oracle_with_all_ones_masks_is_the_plain_unet_oracle():
    from oracle import sggan_oracle as O
    from tests import unet_oracle as U
    rng = np.random.default_rng(9)
    P = {k: torch.tensor(v, dtype=torch.float64) for k, v in O.init_params(U.unet_param_shapes(8, 3, 3), rng, 0.1).items()}
    x = torch.tensor(rng.uniform(0, 1, (2, 3, 16, 16)), dtype=torch.float64)
    ones = [torch.ones(2, 64, 16, 16, dtype=torch.float64)] * 3
    assert (DO.torch_generator_unet(P, x, ones, 0.0) - U.torch_generator_unet(P, x)).abs().max() < 1e-12
    masks = DO.nchw_masks(1, 19, 0, 0, 2, 16, 16, 64, 0.5)
    assert (DO.torch_generator_unet(P, x, masks, 0.5) - U.torch_generator_unet(P, x)).abs().max() > 1e-3


# ----------------------------------------------------------------------------- the library, without a GPU
def test_header_declares_and_binding_binds_the_export():
    src = open(os.path.join(ROOT, "include", "sggan.h")).read()
    assert re.search(r"int sgg_dropout\(void\* x, int64_t n_samples, int64_t elems_per_sample, int threshold,", src)
    assert "sgg_dropout" in A.SIGNATURES and hasattr(ctypes.CDLL(A.LIB_PATH), "sgg_dropout")
    assert "dropout.hip" in open(os.path.join(ROOT, "sg-gan-tf2_amd", "build.py")).read()


def test_argument_checks_are_answered_before_any_launch():
    """Every SGG_EINVAL / SGG_EUNSUPPORTED case of include/sggan.h and the n_samples == 0 no-op: none of them touches the device
    (the pointers are never dereferenced on the host)."""
    L = A.lib()
    x, it = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    call = lambda x=x, n=0, e=64, thr=32768, it=it, off=0, sid=0, dtype=A.SGG_BF16: L.sgg_dropout(x, n, e, thr, it, 19, off, sid, dtype, None)
    assert call() == A.OK                                                    # n_samples == 0: a no-op
    assert call(dtype=A.SGG_F32, sid=2 ** 28 - 1, thr=65535, e=2 ** 35) == A.OK
    for kw in (dict(x=None), dict(it=None), dict(n=-1), dict(e=-8), dict(e=12), dict(x=ctypes.c_void_p(0x1008)), dict(thr=-1),
               dict(thr=65536), dict(sid=-1), dict(sid=2 ** 28), dict(off=-1), dict(dtype=A.SGG_U8), dict(dtype=7)):
        assert call(**kw) == A.EINVAL, kw
    assert call(e=2 ** 35 + 8) == A.EUNSUPPORTED                             # the vector index must fit 32 bits
    assert call(n=65536) == A.EUNSUPPORTED                                   # a grid past the launch limit
    assert call(n=3, thr=0) == A.OK                                          # threshold 0: every bit kept, nothing launched


# ----------------------------------------------------------------------------- flag and constructor
def test_flag_is_absent_unless_given_and_bare_flag_is_the_references_rate():
    from sggan_amd.main import parse_args
    assert not hasattr(parse_args(["--generator", "unet"]), "dropout")
    assert parse_args(["--generator", "unet", "--dropout"]).dropout == 0.5
    assert parse_args(["--generator", "unet", "--dropout", "0.2"]).dropout == 0.2
    assert sggan_amd.default_args().dropout is None


@pytest.mark.parametrize("rate", [-0.1, 1.0, 2.0])
def test_bad_rates_are_refused(rate):
    with pytest.raises(ValueError, match="dropout"):
        sggan_amd.sggan(sggan_amd.default_args(use_resnet=False, dropout=rate))


def test_resnet_generator_refuses_the_option():
    with pytest.raises(ValueError, match="no dropout layers"):
        sggan_amd.sggan(sggan_amd.default_args(use_resnet=True, dropout=0.5))


def test_kernel_resources(tmp_path):
    """csrc/dropout.hip recompiled with -Rpass-analysis=kernel-resource-usage: a streaming kernel -- no spills, no scratch, no
    LDS.  Recorded from the build: f32 62 VGPRs, bf16 40 VGPRs (four vectors in flight per thread), occupancy 8 waves per SIMD."""
    usage = kernel_resource_usage("dropout.hip", tmp_path)
    for frag, vgpr in (("dropout_kernelIfE", 64), ("dropout_kernelIDF16bE", 48)):
        u = the_kernel(usage, frag)
        print(frag, u)
        assert u["vspill"] == 0 and u["sspill"] == 0 and u["scratch"] == 0 and u["lds"] == 0
        assert u["vgpr"] <= vgpr and u["occ"] == 8
