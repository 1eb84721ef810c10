"""The feature-matching option (``--fm_lambda``) without a GPU: the float64 oracle's term and gradient against torch
autograd on an independent restatement of the taps, the generator gradient of a tiny step against central differences, five planted
errors the GPU comparisons must catch, the ambiguity cap of the GPU step tests' fixed cases on the oracle alone, the emulator against
the plain float64 rule, the flag and the constructor's refusals, the library's argument checks and the kernels' resource usage."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sggan_amd
from oracle import sggan_oracle as O
from oracle import torch_restatement as T
from sggan_amd import _abi as A
from sggan_amd import kernels as K
from tests import composed_oracle as CO
from tests import featmatch_oracle as FO
from tests.kernel_resources import kernel_resource_usage, the_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
def _torch_taps(P, x, leak=0.3, eps=1e-3):
    """The seven taps + the h4 map, torch ops, NCHW, float64 (oracle.torch_restatement.discriminator with its intermediates)."""
    h = F.leaky_relu(T.conv2d(x, P["h0_w"], P["h0_b"], 2, "SAME"), leak)
    out = [h]
    for n, s, p in FO._TAIL:
        h = F.leaky_relu(T.inorm(T.conv2d(h, P[n + "_w"], P[n + "_b"], s, p), P[n + "_g"], P[n + "_beta"], eps), leak)
        out.append(h)
    return out, T.conv2d(h, P["h4_w"], P["h4_b"], 1, "SAME")


def test_oracle_term_and_gradient_equal_torch_autograd():
    """ndf 4, 1 x 128 x 128 (the 1 x 1 layer included): the term, its gradient w.r.t. the fake image and w.r.t. every parameter of D
    through the fake pass (the reals are constants) against autograd on the torch restatement."""
    rng = np.random.default_rng(7)
    PD = O.init_params(O.discriminator_param_shapes(df_dim=4), rng, 0.1)
    xr, xf = rng.uniform(0, 1, (1, 128, 128, 3)), rng.uniform(0, 1, (1, 128, 128, 3))
    mask = np.stack([O.one_hot(i, 34) for i in rng.integers(0, 34, (1, 1, 1))]).astype(np.float64)
    tape = O.Tape()
    V = {k: O.Var(v, k) for k, v in PD.items()}
    vf = O.Var(xf)
    _, f_real, _ = FO.discriminator(tape, V, O.Var(xr), mask)
    n_real = len(tape.ops)
    _, f_fake, _ = FO.discriminator(tape, V, vf, mask)
    term = FO.feature_match(tape, f_real, f_fake)
    tape.backward([(term, 1.0)])
    assert all(out.g is None for out, _ in tape.ops[:n_real])                # nothing reaches the real pass
    Pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in PD.items()}
    tf = torch.tensor(xf, dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_(True)
    with torch.no_grad():
        t_real, _ = _torch_taps(Pt, torch.tensor(xr, dtype=torch.float64).permute(0, 3, 1, 2))
    t_fake, _ = _torch_taps(Pt, tf)
    tt = sum((a - b).abs().mean() for a, b in zip(t_fake, t_real)) / 7
    tt.backward()
    print(f"term: oracle {float(term.v):.12f} torch {tt.item():.12f}")
    assert abs(float(term.v) - tt.item()) < 1e-12 and float(term.v) > 1e-3
    assert (f_fake[6].v == f_real[6].v).all() and f_fake[6].v.shape == (1, 1, 1, 32)          # the degenerate layer: beta on both sides
    gx = tf.grad.permute(0, 2, 3, 1).numpy()
    assert np.abs(vf.g - gx).max() < 1e-10 * np.abs(gx).max() + 1e-16 and np.abs(gx).max() > 0
    for k, v in V.items():
        g = Pt[k].grad.numpy() if Pt[k].grad is not None else np.zeros_like(v.v)
        got = np.zeros_like(v.v) if v.g is None else v.g
        assert np.abs(got - g).max() <= 1e-9 * max(np.abs(g).max(), 1e-6), k


class _Branches(O.KinkPolicy):
    """Records the side every ReLU / LeakyReLU element took (the oracle's own decisions, nothing overridden)."""

    def __init__(self):
        super().__init__(0.0)
        self.taken = []

    def decide(self, pre):
        pos = super().decide(pre)
        self.taken.append(pos.copy())
        return pos


def test_generator_gradient_equals_central_differences():
    """ngf = ndf = 4, one block, 1 x 128 x 128: the directional derivative of gen_loss (with fm_lambda 10) along a random direction
    in the generator's parameters against central differences at step 1e-9, away from sign changes: no sign() argument of the term
    or of the L1 term and no activation changes sides between the two shifted evaluations (asserted), so the difference quotient
    stays on one smooth piece."""
    rng = np.random.default_rng(12)
    PG = O.init_params(O.generator_param_shapes(gf_dim=4, n_blocks=1), rng, 0.1)
    PD = O.init_params(O.discriminator_param_shapes(df_dim=4), rng, 0.1)
    real, seg, mask = CO.case_inputs(rng, 1)

    def step(P, fm_lambda=10.0):
        O.KINKS = _Branches()
        try:
            q = FO.reference_step(P, PD, None, real, seg, mask, fm_lambda=fm_lambda)
            sides = O.KINKS.taken
        finally:
            O.KINKS = None
        sides += [np.sign(f - x) for x, f in zip(q["features"]["real"], q["features"]["fake"])] + [np.sign(seg - q["fake_A"])]
        return q, sides
    r, _ = step(PG)
    d = {k: rng.standard_normal(v.shape) for k, v in PG.items()}
    eps = 1e-9
    (rp, sp), (rm, sm) = step({k: PG[k] + eps * d[k] for k in PG}), step({k: PG[k] - eps * d[k] for k in PG})
    assert len(sp) == 20 + 8 and all(np.array_equal(a, b) for a, b in zip(sp, sm))
    num = (rp["gen_loss"] - rm["gen_loss"]) / (2 * eps)
    ana = sum(float((r["gG"][k] * d[k]).sum()) for k in d)
    scale = sum(float(np.abs(r["gG"][k] * d[k]).sum()) for k in d)
    print(f"analytic {ana:+.9e}, central differences {num:+.9e}, scale {scale:.3e}")
    assert abs(num - ana) < 1e-6 * scale and scale > 0
    # ... and the term carries weight in it: without it the derivative is another number
    r0, _ = step(PG, 0.0)
    assert abs(sum(float((r0["gG"][k] * d[k]).sum()) for k in d) - ana) > 1e-3 * scale


# ---- planted errors ----------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / max(np.linalg.norm(b), 1e-300))


def test_five_planted_errors_move_the_result_beyond_the_gpu_tolerances():
    """ndf 4 (h0's four channels sit in eight padded ones), 1 x 128 x 128.  The GPU test holds the term to 1e-5, every gradient
    tensor to 2e-4 of its norm and the stored feature gradients to the kernel's rounding."""
    rng = np.random.default_rng(13)
    PG = O.init_params(O.generator_param_shapes(gf_dim=4, n_blocks=1), rng, 0.1)
    PD = O.init_params(O.discriminator_param_shapes(df_dim=4), rng, 0.1)
    inputs = CO.case_inputs(rng, 1)
    step = lambda **kw: FO.reference_step(PG, PD, None, *inputs, fm_lambda=10.0, **kw)
    r = step()
    worst = lambda q, key: max(_rel(q[key][k], v) for k, v in r[key].items())      # (a tensor whose gradient was 0: any change counts)
    q = step(in_disc_loss=True)                                  # the term in D's loss as well
    assert worst(q, "gD") > 2e-4 and worst(q, "gG") == 0.0
    q = step(count_pad=K.cpad)                                   # count_i over the padded channels
    assert abs(q["fm_loss"] - r["fm_loss"]) > 1e-5 * r["fm_loss"] and _rel(q["fm_grads"][0], r["fm_grads"][0]) > 0.4
    q = step(with_logits=True)                                   # the logit map as an eighth feature
    assert abs(q["fm_loss"] - r["fm_loss"]) > 1e-5 * r["fm_loss"] and worst(q, "gG") > 2e-4 and len(q["fm_grads"]) == 8
    q = step(layer_sum=True)                                     # the sum over the layers
    assert abs(q["fm_loss"] - 7 * r["fm_loss"]) < 1e-12 and worst(q, "gG") > 2e-4
    q = step(sign0=1.0)                                          # sign(0) = +1: only the 1 x 1 layer has zeros
    assert not r["fm_grads"][6].any() and np.allclose(q["fm_grads"][6], 10.0 / (7 * 32), rtol=1e-14, atol=0)
    assert all(np.array_equal(a, b) for a, b in zip(q["fm_grads"][:6], r["fm_grads"][:6]))


# ---- the GPU step tests' cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FO.CASES))
def test_ambiguity_cap_of_the_fixed_cases(name):
    """At most 0.5 % of the term's sign arguments lie within 1e-4 of zero, on the oracle's own features.  Measured: resnet 172 of
    155008 (128 of them the exact zeros of the 1 x 1 layer), unet 164 of 155008 (128), composed 111 of 155008 (0: no instance
    norm), resnet160 66 of 341632 (0: h33's map is 2 x 4)."""
    spec, P, U, inputs = FO.case(name)
    r = FO.case_step(name, P, U, inputs)
    n, amb, zeros = FO.sign_counts(r["features"], FO.MARGIN)
    print(f"{name}: {amb} of {n} within {FO.MARGIN} of zero ({100.0 * amb / n:.2f} %), {zeros} exactly zero")
    assert n == (341632 if name == "resnet160" else 155008) and amb <= FO.CAP * n
    assert zeros == (128 if (spec["H"], spec["W"], spec["spectral"]) == (128, 128, False) else 0)


# ---- the emulator and the plain rule -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
def test_emulator_states_the_float64_rule(bf16):
    rng = np.random.default_rng(17)
    shapes, crs = [(3, 5, 7, 8), (1, 4, 4, 16), (2, 1, 1, 8), (1, 70, 70, 8)], [4, 16, 8, 8]
    mk = lambda s, c: (lambda a: FO.bf16(a) if bf16 else a)((rng.standard_normal(s) * (np.arange(s[-1]) < c)).astype(np.float32))
    reals, fakes = [mk(s, c) for s, c in zip(shapes, crs)], [mk(s, c) for s, c in zip(shapes, crs)]
    fakes[1][0, :2] = reals[1][0, :2]                                        # equal elements
    term, loss, grads, chunks = FO.emulate(reals, fakes, crs, 2.5, bf16, loss=1.25)
    t64, l64, g64 = K.feature_match_ref(reals, fakes, crs, 2.5, loss=1.25, bf16=bf16)
    assert chunks == ([1, 1, 1, 2] if bf16 else [1, 1, 1, 3])
    assert abs(float(term) - float(t64)) <= np.spacing(np.float32(t64)) and abs(float(loss) - float(l64)) <= np.spacing(np.float32(l64))
    for a, b in zip(grads, g64):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not grads[0][..., 4:].any() and not np.signbit(grads[0][..., 4:]).any() and not grads[1][0, :2].any()
    same = FO.emulate(reals, reals, crs, 2.5, bf16)
    assert same[0] == 0.0 and same[1] == 0.0 and not any(g.any() or np.signbit(g).any() for g in same[2])


# ---- flag, refusals ----------------------------------------------------------------------------------------------------------------
def test_flag_is_absent_unless_given(capsys):
    from sggan_amd.main import parse_args
    assert not hasattr(parse_args([]), "fm_lambda") and parse_args(["--fm_lambda", "10"]).fm_lambda == 10.0
    with pytest.raises(SystemExit):
        parse_args(["--fm_lambda"])
    capsys.readouterr()
    assert sggan_amd.default_args().fm_lambda == 0.0


@pytest.mark.parametrize("kw,match", [(dict(fm_lambda=1.0, cycle=True), "no pixel-aligned real"),
                                      (dict(fm_lambda=1.0, diffaug="color"), "independent draws"),
                                      (dict(fm_lambda=-1.0), "fm_lambda must be finite and >= 0"),
                                      (dict(fm_lambda=float("nan")), "fm_lambda must be finite and >= 0")])
def test_constructor_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        sggan_amd.sggan(sggan_amd.default_args(**kw))


def test_zero_is_off():
    """fm_lambda = 0 (or None) is off: the two refusals that fm_lambda = 1 meets with --cycle and with --diffaug are not raised -- the
    constructor goes on to its next check (here: the device) -- and the model without the argument in its namespace is the same."""
    for kw in (dict(cycle=True), dict(diffaug="color")):
        with pytest.raises(ValueError, match="fm_lambda"):
            sggan_amd.sggan(sggan_amd.default_args(fm_lambda=1.0, device="cpu", **kw))
        for v in (0.0, None, 0):
            with pytest.raises(NotImplementedError, match="no host implementation"):
                sggan_amd.sggan(sggan_amd.default_args(fm_lambda=v, device="cpu", **kw))
    args = sggan_amd.default_args(cycle=True, device="cpu")
    del args.fm_lambda
    with pytest.raises(NotImplementedError, match="no host implementation"):
        sggan_amd.sggan(args)


# ---- the library, without a GPU ----------------------------------------------------------------------------------------------------
def test_symbols_struct_and_constants():
    src = open(os.path.join(ROOT, "include", "sggan.h")).read()
    lib = ctypes.CDLL(A.LIB_PATH)
    for name in ("sgg_feature_match", "sgg_feature_match_workspace"):
        assert name + "(const sgg_fm_pair* pairs, int L," in src and name in A.SIGNATURES and hasattr(lib, name)
    assert "#define SGG_FM_MAX_PAIRS 8" in src and A.FM_MAX_PAIRS == 8 and ctypes.sizeof(A.FmPair) == 40
    assert "featmatch.hip" in open(os.path.join(ROOT, "sg-gan-tf2_amd", "build.py")).read()
    srck = open(os.path.join(ROOT, "sg-gan-tf2_amd", "csrc", "featmatch.hip")).read()
    assert "constexpr int FM_THREADS = 256;" in srck and "constexpr int FM_CHUNK = 4096;" in srck
    assert (K.FEATMATCH_THREADS, K.FEATMATCH_CHUNK) == (FO.THREADS, FO.CHUNK) == (256, 4096)
    assert "atomic" not in srck.replace("No atomics", "")


def test_argument_checks_are_answered_before_any_launch():
    L = A.lib()
    p = lambda real=0x1000, fake=0x2000, grad=0x3000, P=16, C_real=8, Cpad=8: A.FmPair(real, fake, grad, P, C_real, Cpad)
    arr = lambda *ps: (A.FmPair * len(ps))(*ps)
    loss, term, ws = ctypes.c_void_p(0x4000), ctypes.c_void_p(0x5000), ctypes.c_void_p(0x6000)
    call = lambda pairs, n, loss=loss, term=term, dtype=A.SGG_F32, ws=ws, nb=1 << 20: L.sgg_feature_match(pairs, n, 1.0, loss, term, 0, dtype, ws, nb, None)
    one = arr(p())
    assert call(None, 1) == A.EINVAL and call(one, 0) == A.EINVAL and call(arr(*[p()] * 9), 9) == A.EINVAL
    assert call(one, 1, loss=None) == A.EINVAL and call(one, 1, term=None) == A.EINVAL
    assert call(one, 1, dtype=A.SGG_U8) == A.EINVAL and call(one, 1, dtype=7) == A.EINVAL
    for bad in (dict(real=None), dict(fake=None), dict(grad=None), dict(real=0x1008), dict(grad=0x3004), dict(P=0), dict(P=-1), dict(Cpad=12),
                dict(Cpad=4, C_real=4), dict(Cpad=0, C_real=0), dict(C_real=0), dict(C_real=9)):
        assert call(arr(p(), p(**bad)), 2) == A.EINVAL, bad
    assert call(arr(p(P=2 ** 30)), 1) == A.EUNSUPPORTED                      # 2^31 vectors of four floats: one past the 32-bit index
    assert call(arr(p(P=2 ** 30 - 1)), 1, nb=8) == A.EWORKSPACE
    assert call(one, 1, ws=None) == A.EWORKSPACE and call(one, 1, nb=7) == A.EWORKSPACE and call(one, 1, ws=ctypes.c_void_p(0x6004)) == A.EWORKSPACE
    q = L.sgg_feature_match_workspace
    assert q(one, 1, A.SGG_F32) == 8 and q(arr(p(P=4097)), 1, A.SGG_F32) == 24 and q(arr(p(P=4097)), 1, A.SGG_BF16) == 16
    assert q(arr(*[p(real=None, fake=None, grad=None)] * 8), 8, A.SGG_BF16) == 64         # (the query reads no pointer)
    assert q(one, 0, A.SGG_F32) == 0 and q(None, 1, A.SGG_F32) == 0 and q(arr(p(Cpad=12)), 1, A.SGG_F32) == 0


def test_wrapper_checks_shapes_and_dtypes():
    t = lambda *s, d=torch.float32: torch.zeros(s, dtype=d)
    for reals, fakes, crs in (([], [], []), ([t(2, 8)] * 9, [t(2, 8)] * 9, [8] * 9), ([t(2, 8)], [t(3, 8)], [8]), ([t(2, 8)], [t(2, 8)], [8, 8]),
                              ([t(2, 12)], [t(2, 12)], [12]), ([t(2, 8)], [t(2, 8)], [9]), ([t(2, 8)], [t(2, 8)], [0]), ([t(0, 8)], [t(0, 8)], [8]),
                              ([t(2, 8)], [t(2, 8, d=torch.bfloat16)], [8]),
                              ([t(2, 8), t(2, 8, d=torch.bfloat16)], [t(2, 8), t(2, 8, d=torch.bfloat16)], [8, 8])):
        with pytest.raises(ValueError, match="feature_match"):
            K.feature_match(reals, fakes, crs, t(1), t(1), 1.0)
    # tensors the kernel could not walk are refused before any address is taken: host memory, a strided view, a wrong scalar
    for reals, fakes, loss in (([t(2, 8)], [t(2, 8)], t(1)), ([t(2, 16)[:, :8]], [t(2, 8)], t(1)), ([t(2, 8)], [t(2, 8)], t(2))):
        with pytest.raises(ValueError, match="feature_match"):
            K.feature_match(reals, fakes, [8], loss, t(1), 1.0)
    with pytest.raises(ValueError, match="feature_match: out"):
        K.feature_match([t(2, 8)], [t(2, 8)], [8], t(1), t(1), 1.0, out=[t(3, 8)])
    with pytest.raises(ValueError, match="feature_match"):
        sggan_amd.feature_match([t(2, 4)], [t(2, 5)])


def test_kernel_resources(tmp_path):
    """csrc/featmatch.hip recompiled with -Rpass-analysis=kernel-resource-usage: no spilled VGPR or SGPR and no scratch in the
    streaming kernel (f32 and bf16) and in the fold -- the by-value table is read with static indices only.  Recorded from the
    build: 58 / 66 VGPRs and 32 bytes of LDS (the four waves' doubles) in the streaming kernel; the fold keeps a 4 KB tile of partials
    and the eight layer means in LDS, 63 VGPRs."""
    usage = kernel_resource_usage("featmatch.hip", tmp_path)
    kernels = [the_kernel(usage, "fm_partial_kernelIfE"), the_kernel(usage, "fm_partial_kernelIDF16bE"), the_kernel(usage, "fm_fold_kernel")]
    assert len(usage) == 3
    for u in kernels:
        print(u)
        assert u["vspill"] == 0 and u["sspill"] == 0 and u["scratch"] == 0
        assert u["vgpr"] <= 96 and u["occ"] >= 5
    assert all(u["lds"] == 32 for u in kernels[:2]) and kernels[2]["lds"] == 512 * 8 + 64
