"""The resize-convolution option of generator_resnet without a GPU: the float64 oracle of the 2x resampling against
torch's interpolate, the adjoint identity, the oracle generator against an independent torch restatement and its gradients against
central differences, five planted errors those comparisons must catch, the library's argument checks (answered before any launch),
the flag, the parameter specs, the constructor's refusals, and the kernels' resource usage."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sggan_amd
from oracle import sggan_oracle as O
from oracle import torch_restatement as T
from sggan_amd import _abi as A
from sggan_amd import kernels as K
from tests import upsample_oracle as UO
from tests.kernel_resources import kernel_resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 2), (2, 1), (3, 5), (4, 7)]


def _interp(x, mode):
    """torch's statement of U on an NHWC float64 array."""
    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    kw = {} if mode == "nearest" else {"align_corners": False}
    return F.interpolate(t, scale_factor=2, mode=mode, **kw).permute(0, 2, 3, 1).numpy()


def _fwd_err(up):
    """max |up(x) - interpolate(x)| over the sizes and both modes."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for H, W in SIZES:
        x = rng.standard_normal((2, H, W, 3))
        for mode in UO.MODES:
            worst = max(worst, float(np.abs(up(x, mode) - _interp(x, mode)).max()))
    return worst


def _adjoint_err(up, up_T):
    """max |<U x, g> - <x, U^T g>| / (|x| |g|) over the sizes and both modes."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for H, W in SIZES:
        x, g = rng.standard_normal((2, H, W, 3)), rng.standard_normal((2, 2 * H, 2 * W, 3))
        for mode in UO.MODES:
            worst = max(worst, abs(float((up(x, mode) * g).sum() - (x * up_T(g, mode)).sum())) / (np.linalg.norm(x) * np.linalg.norm(g)))
    return worst


def test_oracle_forward_is_interpolate():
    err = _fwd_err(UO.up)
    print(f"oracle U against torch.nn.functional.interpolate: {err:.1e}")
    assert err < 1e-14


def test_oracle_adjoint_identity():
    err = _adjoint_err(UO.up, UO.up_T)
    print(f"<U x, g> - <x, U^T g>, relative: {err:.1e}")
    assert err < 1e-14


def test_emulators_state_the_oracle():
    """The kernels' tap order in f32 (tests/upsample_oracle.emulate_*) is the same operator: inside the derived bound of the float64
    one on random inputs, and EXACTLY it -- in bf16 as well -- on the integer inputs the bitwise GPU tests use."""
    rng = np.random.default_rng(3)
    for H, W in SIZES:
        xi = rng.integers(-15, 16, (2, H, W, 8)).astype(np.float32)
        gi = rng.integers(-3, 4, (2, 2 * H, 2 * W, 8)).astype(np.float32)
        xr, gr = rng.standard_normal((2, H, W, 8)).astype(np.float32), rng.standard_normal((2, 2 * H, 2 * W, 8)).astype(np.float32)
        for mode in UO.MODES:
            for bf16 in (False, True):
                assert np.array_equal(UO.emulate_fwd(xi, mode, bf16), UO.up(xi, mode))
                assert np.array_equal(UO.emulate_bwd(gi, mode, bf16), UO.up_T(gi, mode))
                assert np.abs(UO.up_T(gi, mode)).max() <= 12.0
                for emu, direction, v in ((UO.emulate_fwd, "fwd", xr), (UO.emulate_bwd, "bwd", gr)):
                    v = UO._bf16(v) if bf16 else v
                    if (mode, direction) == ("nearest", "fwd"):
                        assert np.array_equal(emu(v, mode, bf16), UO.up(v, mode))
                        continue
                    exact, bnd = UO.bound(v, mode, direction, bf16)
                    assert (np.abs(emu(v, mode, bf16) - exact) <= bnd).all()


# ----------------------------------------------------------------------------- the generator
def _params(rng, ngf, n_blocks):
    return O.init_params(UO.generator_param_shapes(ngf, 3, 3, n_blocks), rng, 0.1)


def _torch_generator(P, x, mode, n_blocks, eps=1e-3, layout="in_out", u_first=True):
    """An independent statement of the resize generator: torch ops, NCHW, float64.  layout / u_first plant errors."""
    P = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in P.items()}
    h = torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2)
    cin = lambda n, h, **kw: T.inorm(T.conv2d(h, P[n + "_w"], P[n + "_b"], **kw), P[n + "_g"], P[n + "_beta"], eps)
    h = F.relu(cin("c1", h, reflect=3))
    h = F.relu(cin("c2", h, stride=2, padding="SAME"))
    h = F.relu(cin("c3", h, stride=2, padding="SAME"))
    for i in range(1, n_blocks + 1):
        y = F.relu(cin(f"r{i}a", h, reflect=1))
        h = cin(f"r{i}b", y, reflect=1) + h
    U = lambda t: F.interpolate(t, scale_factor=2, mode=mode, **({} if mode == "nearest" else {"align_corners": False}))
    for n in ("d1", "d2"):
        w = P[n + "_w"]
        if layout == "out_in":              # the transposed layer's layout read from the same buffer
            w = w.reshape(3, 3, w.shape[3], w.shape[2]).permute(0, 1, 3, 2)
        c = T.conv2d(U(h), w, P[n + "_b"], padding="SAME") if u_first else U(T.conv2d(h, w, P[n + "_b"], padding="SAME"))
        h = F.relu(T.inorm(c, P[n + "_g"], P[n + "_beta"], eps))
    return torch.tanh(T.conv2d(h, P["out_w"], P["out_b"], reflect=3)).permute(0, 2, 3, 1).numpy()


def _oracle_generator(P, x, mode, n_blocks):
    tape = O.Tape()
    V = {k: O.Var(v, k) for k, v in P.items()}
    xv = O.Var(x)
    return UO.generator_resnet_resize(tape, V, xv, mode, n_blocks), tape, V, xv


def _gen_err(mode, **planted):
    rng = np.random.default_rng(4)
    P, x = _params(rng, 4, 1), rng.uniform(0, 1, (2, 8, 8, 3))
    return float(np.abs(_oracle_generator(P, x, mode, 1)[0].v - _torch_generator(P, x, mode, 1, **planted)).max())


@pytest.mark.parametrize("mode", UO.MODES)
def test_oracle_generator_is_the_torch_restatement(mode):
    err = _gen_err(mode)
    print(f"generator_resnet_resize[{mode}] against the torch restatement: {err:.1e}")
    assert err < 1e-12


@pytest.mark.parametrize("mode", UO.MODES)
def test_oracle_generator_gradients_equal_central_differences(mode):
    """ngf 4, one block, 2x8x8: the tape's gradient of <G(x), R> along random directions -- all parameters, d1_w alone, d2_w alone, the
    input alone -- against central differences at step 1e-6, to 1e-6 of the directional derivative's scale."""
    rng = np.random.default_rng(5)
    P, x = _params(rng, 4, 1), rng.uniform(0, 1, (2, 8, 8, 3))
    R = rng.standard_normal((2, 8, 8, 3))
    out, tape, V, xv = _oracle_generator(P, x, mode, 1)
    tape.backward([(out, R)])
    grads = dict({k: v.g for k, v in V.items()}, x=xv.g)
    loss = lambda P_, x_: float((_oracle_generator(P_, x_, mode, 1)[0].v * R).sum())
    for which in (None, "d1_w", "d2_w", "x"):
        d = {k: (rng.standard_normal(np.shape(v)) if which in (None, k) else np.zeros(np.shape(v))) for k, v in dict(P, x=x).items()}
        eps = 1e-6
        shift = lambda s: loss({k: P[k] + s * eps * d[k] for k in P}, x + s * eps * d["x"])
        num = (shift(+1) - shift(-1)) / (2 * eps)
        ana = sum(float((grads[k] * d[k]).sum()) for k in d)
        scale = sum(float(np.abs(grads[k] * d[k]).sum()) for k in d)
        print(f"[{mode}] direction {which or 'all'}: analytic {ana:+.9e}, central differences {num:+.9e}")
        assert abs(num - ana) < 1e-6 * scale and scale > 0


# ----------------------------------------------------------------------------- planted errors
def _wrong_parity(x, mode):
    """bilinear with the weights of the even and the odd outputs exchanged."""
    if mode == "nearest":
        return UO.up(x, mode)
    y = UO.up(x, mode)
    for ax in (1, 2):
        n = y.shape[ax] // 2
        idx = np.arange(2 * n) ^ 1
        y = np.take(y, idx, axis=ax)
    return y


def _no_clamp(x, mode):
    """bilinear with zeros beyond the border instead of the clamped tap."""
    if mode == "nearest":
        return UO.up(x, mode)
    N, H, W, C = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    return UO.up(xp, mode)[:, 2:2 * H + 2, 2:2 * W + 2]


def _adjoint_without_edges(g, mode):
    """U^T with the clamped contributions dropped: the interior formula with zeros beyond the border."""
    if mode == "nearest":
        return UO.up_T(g, mode)
    N, H2, W2, C = g.shape
    gp = np.pad(g, ((0, 0), (2, 2), (2, 2), (0, 0)))
    return UO.up_T(gp, mode)[:, 1:H2 // 2 + 1, 1:W2 // 2 + 1]


def test_planted_errors_are_caught():
    """Each comparison above, handed a wrong statement, reports a distance far above its bar."""
    assert _fwd_err(_wrong_parity) > 1e-2                                   # the wrong parity weight
    assert _fwd_err(_no_clamp) > 1e-2                                       # the missing edge clamp
    assert _adjoint_err(UO.up, _adjoint_without_edges) > 1e-3               # the adjoint's edge term dropped
    # (the planted operators are themselves right in the interior: what the comparisons catch is the planted part)
    rng = np.random.default_rng(6)
    x = rng.standard_normal((1, 6, 6, 2))
    assert np.abs(_no_clamp(x, "bilinear") - UO.up(x, "bilinear"))[:, 2:-2, 2:-2].max() < 1e-14
    g = rng.standard_normal((1, 12, 12, 2))
    assert np.abs(_adjoint_without_edges(g, "bilinear") - UO.up_T(g, "bilinear"))[:, 1:-1, 1:-1].max() < 1e-14
    for mode in UO.MODES:
        assert _gen_err(mode, layout="out_in") > 1e-3                       # (out,in) in place of (in,out)
        assert _gen_err(mode, u_first=False) > 1e-3                         # U applied after the conv


# ----------------------------------------------------------------------------- the library, without a GPU
def test_header_declares_and_binding_binds_the_exports():
    src = open(os.path.join(ROOT, "include", "sggan.h")).read()
    lib = ctypes.CDLL(A.LIB_PATH)
    for name, args in (("sgg_upsample2x_fwd", r"const void\* x, void\* y"), ("sgg_upsample2x_bwd", r"const void\* dy, void\* dx")):
        assert re.search(rf"int {name}\({args}, int N, int H, int W, int Cp, int mode, int dtype, void\* stream\);", src)
        assert name in A.SIGNATURES and hasattr(lib, name)
    assert "SGG_UPSAMPLE_NEAREST = 0, SGG_UPSAMPLE_BILINEAR = 1" in src and (A.UPSAMPLE_NEAREST, A.UPSAMPLE_BILINEAR) == (0, 1)
    assert "upsample.hip" in open(os.path.join(ROOT, "sg-gan-tf2_amd", "build.py")).read()
    srck = open(os.path.join(ROOT, "sg-gan-tf2_amd", "csrc", "upsample.hip")).read()
    consts = tuple(int(re.search(rf"constexpr int {c} = (\w+);", srck).group(1).replace("UP_THREADS", "256")) for c in ("UP_THREADS", "UP_CHUNK", "UP_GRID_BLOCKS"))
    assert consts == (K.UPSAMPLE_THREADS, K.UPSAMPLE_CHUNK, K.UPSAMPLE_GRID_BLOCKS)


@pytest.mark.parametrize("entry", ["sgg_upsample2x_fwd", "sgg_upsample2x_bwd"])
def test_argument_checks_are_answered_before_any_launch(entry):
    """Every SGG_EINVAL / SGG_EUNSUPPORTED case of include/sggan.h and the zero-extent no-op: none touches the device (the pointers
    are never dereferenced on the host)."""
    fn = getattr(A.lib(), entry)
    a, b = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    call = lambda a=a, b=b, N=0, H=4, W=4, Cp=8, mode=0, dtype=A.SGG_BF16: fn(a, b, N, H, W, Cp, mode, dtype, None)
    assert call() == A.OK and call(N=1, H=0) == A.OK and call(N=1, W=0, mode=1, dtype=A.SGG_F32) == A.OK and call(N=1, Cp=0) == A.OK
    for kw in (dict(a=None), dict(b=None), dict(N=-1), dict(H=-1), dict(W=-1), dict(Cp=-8), dict(Cp=12), dict(Cp=4),
               dict(a=ctypes.c_void_p(0x1008)), dict(b=ctypes.c_void_p(0x2004)), dict(mode=2), dict(mode=-1), dict(dtype=A.SGG_U8), dict(dtype=7)):
        assert call(**kw) == A.EINVAL, kw
    assert call(N=2 ** 16, H=2 ** 8, W=2 ** 7, Cp=8) == A.EUNSUPPORTED           # 2^31 low-resolution vectors: one past the 32-bit item index
    assert call(N=2 ** 30, H=2 ** 30, W=2 ** 30, Cp=2 ** 30) == A.EUNSUPPORTED   # (a product past 2^63)


def test_wrappers_refuse_unknown_modes():
    for bad in ("deconv", "cubic", None, 1):
        with pytest.raises(ValueError, match="mode"):
            K.upsample_mode(bad)
    assert [K.upsample_mode(m) for m in UO.MODES] == [0, 1]


# ----------------------------------------------------------------------------- flag, specs, constructor
def test_flag_is_absent_unless_given_and_bad_values_are_refused(capsys):
    from sggan_amd.main import parse_args
    assert not hasattr(parse_args([]), "upsample")
    for v in ("deconv", "nearest", "bilinear"):
        assert parse_args(["--upsample", v]).upsample == v
    for bad in (["--upsample", "bicubic"], ["--upsample"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    capsys.readouterr()
    assert sggan_amd.default_args().upsample == "deconv"


def test_param_specs_keep_names_order_and_sizes():
    from sggan_amd.module import generator_param_specs, ParamStore
    base = generator_param_specs(64, 3, 3, 9)
    assert base == generator_param_specs(64, 3, 3, 9, "deconv")
    for mode in UO.MODES:
        specs = generator_param_specs(64, 3, 3, 9, mode)
        shapes = dict(specs)
        assert shapes["d1_w"] == (3, 3, 256, 128) and shapes["d2_w"] == (3, 3, 128, 64)                  # Conv2D: (kh,kw,in,out)
        assert dict(base)["d1_w"] == (3, 3, 128, 256) and dict(base)["d2_w"] == (3, 3, 64, 128)          # transposed: (kh,kw,out,in)
        assert [n for n, _ in specs] == [n for n, _ in base]
        assert [int(np.prod(s)) for _, s in specs] == [int(np.prod(s)) for _, s in base]
        assert {n: s for n, s in specs if n not in ("d1_w", "d2_w")} == {n: s for n, s in base if n not in ("d1_w", "d2_w")}
        a, b = ParamStore(specs, "cpu"), ParamStore(base, "cpu")
        assert a.numel == b.numel and {k: v[:2] for k, v in a.index.items()} == {k: v[:2] for k, v in b.index.items()}
        assert [(n, tuple(s)) for n, s in generator_param_specs(8, 3, 3, 2, mode)] == [(n, tuple(s)) for n, s in UO.generator_param_shapes(8, 3, 3, 2)]
        # the Glorot limit is symmetric in the two fans: the same seed draws the same buffer
        a.init_keras(19); b.init_keras(19)
        assert torch.equal(a.flat, b.flat)
    with pytest.raises(ValueError, match="upsample"):
        generator_param_specs(upsample="cubic")


def test_unet_generator_refuses_the_option():
    for mode in UO.MODES:
        with pytest.raises(ValueError, match="no stride-2 layer"):
            sggan_amd.sggan(sggan_amd.default_args(use_resnet=False, upsample=mode))


@pytest.mark.parametrize("bad", ["cubic", "Nearest", 2])
def test_values_outside_the_three_are_refused(bad):
    with pytest.raises(ValueError, match="upsample"):
        sggan_amd.sggan(sggan_amd.default_args(upsample=bad))


def test_kernel_resources(tmp_path):
    """csrc/upsample.hip recompiled with -Rpass-analysis=kernel-resource-usage: streaming kernels -- no VGPR or SGPR spill, no
    scratch, no LDS, in all eight instantiations (forward / adjoint x nearest / bilinear x f32 / bf16).  Recorded from the build:
    20-38 VGPRs for nearest, 64-86 for bilinear; at least 5 waves per SIMD."""
    usage = {k: v for k, v in kernel_resource_usage("upsample.hip", tmp_path).items() if "upsample2x_" in k}
    assert len(usage) == 8 and sum("fwd" in k for k in usage) == 4 and sum("IDF16b" in k for k in usage) == 4
    for name, u in usage.items():
        print(name, u)
        assert u["vspill"] == 0 and u["sspill"] == 0 and u["scratch"] == 0 and u["lds"] == 0
        assert u["vgpr"] <= 96 and u["occ"] >= 5
