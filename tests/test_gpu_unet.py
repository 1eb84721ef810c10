"""generator_unet (reference module.py:125-206) on the MI355X path: its layer shapes bit-exact on integer inputs, the
skip-before-activation instance norm against float64, the reference-mode step against the float64 U-Net oracle
(tests/unet_oracle.py), the bf16 step, HIP-graph replay, checkpoints and the CLI."""
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import sggan_oracle as O
from tests import unet_oracle as U
from tests.test_gpu_exact import dev, ints, same, store
from tests.test_gpu_step import _l2, _rand_inputs, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


# (name, kind, Cin, Cout): the U-Net's distinct 3x3 stride-1 'same' layer shapes
LAYERS = [("e5_512_512", "conv", 512, 512), ("e4_256_512", "conv", 256, 512), ("d1_T_512_512", "deconv", 512, 512),
          ("d5_T_512_256", "deconv", 512, 256), ("d7_T_128_64", "deconv", 128, 64), ("e1_3_64", "conv", 3, 64),
          ("d8_T_64_3", "deconv", 64, 3)]


@pytest.mark.parametrize("hw", [128, 64], ids=["128px", "64px"])
@pytest.mark.parametrize("layer", LAYERS, ids=[l[0] for l in LAYERS])
def test_unet_layer_fwd_bwd_bit_exact(sg, layer, hw):
    """Integer inputs (tests/test_gpu_exact.py): forward, data gradient and weight / bias gradient equal the float64 oracle bit for
    bit after the one rounding to the storage dtype.  128 px: the halo GEMM kernels (W % 128 == 0); 64 px: the generic GEMM."""
    name, kind, Ci, Co = layer
    N = 2
    rng = np.random.default_rng(zlib.crc32((name + str(hw)).encode()))
    x = ints(rng, (N, hw, hw, Ci))
    b = ints(rng, (Co,), -2, 2)
    w = ints(rng, (3, 3, Ci, Co) if kind == "conv" else (3, 3, Co, Ci))
    t = O.Tape()
    vx, vw, vb = O.Var(x), O.Var(w), O.Var(b)
    y = O.conv2d(t, vx, vw, vb, 1, "SAME") if kind == "conv" else O.deconv2d(t, vx, vw, vb, stride=1)
    dy = ints(rng, y.v.shape)
    t.backward([(y, dy)])
    assert max(np.abs(y.v).max(), np.abs(vx.g).max(), np.abs(vw.g).max()) < 2 ** 24 and np.abs(vw.g).max() > 8
    for dtype in (torch.bfloat16, torch.float32):
        tx = dev(x, dtype).requires_grad_(True)
        tw, tb = dev(w).requires_grad_(True), dev(b).requires_grad_(True)
        ty = sg.conv2d(tx, tw, tb, stride=1, padding="SAME") if kind == "conv" else sg.deconv2d(tx, tw, tb, stride=1)
        tag = f"{name}@{hw}[{str(dtype).split('.')[-1]}]"
        same(ty, store(y.v, dtype), tag + " y")
        ty.backward(dev(dy, dtype))
        same(tx.grad, store(vx.g, dtype), tag + " dx")
        same(tw.grad, vw.g, tag + " dw")
        same(tb.grad, vb.g, tag + " db")


def _skip_norm_oracle(x, gamma, beta, skip, dy, pos, leak, eps=1e-3):
    """float64 y = act(IN(x) + skip) and its backward, with the activation's branch given by ``pos``."""
    mu = x.mean((1, 2), keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean((1, 2), keepdims=True) + eps)
    xh = (x - mu) * rstd
    z = gamma * xh + beta + skip
    y = np.where(pos, z, leak * z)
    dz = dy * np.where(pos, 1.0, leak)
    g = dz * gamma
    dx = rstd * (g - g.mean((1, 2), keepdims=True) - xh * (g * xh).mean((1, 2), keepdims=True))
    return z, y, dz, dx, (dz * xh).sum((0, 1, 2)), dz.sum((0, 1, 2))


@pytest.mark.parametrize("act", ["relu", "lrelu"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_skip_before_activation_norm_matches_float64(sg, dtype, act):
    """sgg_instnorm_fwd_skip / _partial / sgg_instnorm_bwd_skip against float64, with exact zeros planted in the pre-activation
    (gamma = beta = 0 on some channels and skip = 0 at some of their pixels: z = 0 exactly, where act' must be 0 / leak)."""
    from sggan_amd import _abi as A
    from sggan_amd import kernels as K
    N, H, W, C = 2, 24, 40, 64
    code, leak = (A.ACT_RELU, 0.0) if act == "relu" else (A.ACT_LRELU, float(np.float32(0.3)))    # the kernel's f32 slope
    rng = np.random.default_rng(11)
    rnd = lambda a=1.0, b=0.0: store(rng.standard_normal((N, H, W, C)) * a + b, dtype)
    x, skip, dy = rnd(3.0, 1.0), rnd(), rnd()
    gamma, beta = 1 + 0.2 * rng.standard_normal(C), 0.2 * rng.standard_normal(C)
    gamma = gamma.astype(np.float32).astype(np.float64); beta = beta.astype(np.float32).astype(np.float64)
    gamma[::8] = 0.0; beta[::8] = 0.0
    planted = np.zeros((N, H, W, C), bool)
    planted[:, ::3, ::2, ::8] = True
    skip[planted] = 0.0
    tx, ts, tdy = dev(x, dtype), dev(skip, dtype), dev(dy, dtype)
    tg, tb = dev(gamma), dev(beta)
    y, stats = K.instnorm_fwd_skip(tx, tg, tb, ts, 1e-3, code, leak)
    # the partial-sums form with host-made (sum, sumsq) rows: one chunk per image
    xs = tx.to(torch.float64)
    part = torch.stack([xs.sum((1, 2)), (xs * xs).sum((1, 2))], -1)[:, None].to(torch.float32).contiguous()
    y2, _ = K.instnorm_fwd_skip(tx, tg, tb, ts, 1e-3, code, leak, partial=part)
    pos = (y > 0).cpu().numpy()
    z, ye, dz, dxe, dge, dbe = _skip_norm_oracle(x, gamma, beta, skip, dy, pos, leak)
    assert np.all(z[planted] == 0) and not pos[planted].any()
    assert not (pos != (z > 0))[np.abs(z) > 1e-4].any()           # the kernel's branch is the oracle's outside the rounding band
    ftol = 1e-5 if dtype == torch.float32 else 2e-2
    assert rel(y.float().cpu().numpy(), ye) < ftol and rel(y2.float().cpu().numpy(), ye) < ftol
    assert np.all(y.float().cpu().numpy()[planted] == 0)
    dg = torch.full((C,), 0.5, device="cuda"); db = torch.full((C,), -0.5, device="cuda")
    dx, dskip = K.instnorm_bwd_skip(tdy, y, tx, tg, tb, stats, dg, db, accumulate=True, act=code, leak=leak)
    btol = 2e-5 if dtype == torch.float32 else 3e-2
    got_dz = dskip.float().cpu().numpy()
    assert np.array_equal(got_dz, store(dz, dtype))               # dy * act'(y): one multiply by 1 / 0 / leak, one rounding
    assert np.all(got_dz[planted] == (0.0 if act == "relu" else store(leak * dy, dtype)[planted]))
    assert rel(dx.float().cpu().numpy(), dxe) < btol
    assert rel(dg.cpu().numpy() - 0.5, dge) < btol and rel(db.cpu().numpy() + 0.5, dbe) < btol
    # deterministic: a second call writes the same bits
    dx2, dskip2 = K.instnorm_bwd_skip(tdy, y, tx, tg, tb, stats, dg, db, act=code, leak=leak)
    assert torch.equal(dx, dx2) and torch.equal(dskip, dskip2)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _unet_case(sg, ngf, ndf, N, seed, dtype="f32", **kw):
    rng = np.random.default_rng(seed)
    PG = {k: _f32(v) for k, v in O.init_params(U.unet_param_shapes(ngf, 3, 3), rng, 0.1).items()}
    PD = {k: _f32(v) for k, v in O.init_params(O.discriminator_param_shapes(df_dim=ndf), rng, 0.1).items()}
    real, seg = _f32(rng.uniform(0, 1, (N, 128, 128, 3))), _f32(rng.uniform(0, 1, (N, 128, 128, 3)))
    mask = np.stack([O.one_hot(i, 34) for i in rng.integers(0, 34, (N, 4, 4))]).astype(np.float64)
    m = sg.sggan(sg.default_args(use_resnet=False, ngf=ngf, ndf=ndf, dtype=dtype, **kw))
    m.generator.P.load(PG); m.discriminator.P.load(PD)
    m.real_A, m.seg_A, m.mask_A = real.astype(np.float32), seg.astype(np.float32), mask.astype(np.float32)
    return m, (PG, PD, real, seg, mask)


@pytest.mark.parametrize("N", [1, 2])
def test_unet_reference_step_f32_matches_kink_aware_oracle(sg, N):
    """One f32 reference-mode step with the U-Net generator against tests/unet_oracle.train_step evaluated kink-aware.  Bars of
    test_train_step_small_f32_matches_oracle: losses 1e-5, image 1e-4, every gradient 2e-4 (relative L2; single entries 1e-3 of the
    tensor's largest), post-Adam parameters 2e-5.  The generator at the reference's width (ngf 64: 512 channels at full resolution, the halo kernels);
    a narrow discriminator (ndf 8) keeps the float64 oracle's time down."""
    from tests.kink_helpers import discriminator_branches
    m, (PG, PD, real, seg, mask) = _unet_case(sg, 64, 8, N, 100 + N, keep_tapes=True)
    assert type(m.generator).__name__ == "GeneratorUNet" and m.arch == "unet"
    m.train_step()
    gl, dl = m.losses()
    t = m.tapes
    branches = (U.unet_branches(m.generator, t["G"]) + discriminator_branches(m.discriminator, t["D_real"])
                + discriminator_branches(m.discriminator, t["D_fake"]))
    pol = O.KinkPolicy(1e-4, branches)
    O.KINKS = pol
    try:
        r = U.train_step(PG, PD, real, seg, mask)
    finally:
        O.KINKS = None
    print(f"kink-aware U-Net oracle: {pol.elements} decisions, {pol.ambiguous} within 1e-4, {pol.overridden} overridden")
    assert pol.calls == len(branches) and pol.disagree_outside == 0
    assert abs(gl - r["gen_loss"]) < 1e-5 * abs(r["gen_loss"]) and abs(dl - r["disc_loss"]) < 1e-5 * abs(r["disc_loss"])
    assert rel(m.fake_A.numpy(), r["fake_A"]) < 1e-4
    worst = {}
    for label, net, exp, newp, keep in (("gG", m.generator, r["gG"], r["PG"], ("d8_b",)), ("gD", m.discriminator, r["gD"], r["PD"], ("h0_b", "h4_b"))):
        got = net.P.export(net.P.grad)
        for k, v in got.items():
            if k.endswith("_b") and k not in keep:                # bias in front of an InstanceNorm: exactly 0 here
                assert np.abs(v).max() == 0.0 and np.abs(exp[k]).max() < 1e-9
                continue
            worst[(label, k)] = (_l2(v, exp[k]), rel(v, exp[k]))
        ge = exp
        for k, v in net.P.export().items():
            if k.endswith("_b") and k not in keep:
                continue
            sig = np.abs(ge[k]) > 1e-3 * np.abs(ge[k]).max()      # Adam's first step is -lr*g/(|g|+eps): tiny entries may flip
            sig = sig if sig.any() else np.ones_like(sig)          # (an all-zero gradient leaves the tensor as it was)
            assert np.abs(v - newp[k])[sig].max() < 2e-5, (label, "post-Adam", k)
    print("U-Net step, kink-aware: worst gradient tensors (relative L2, worst entry / largest entry):",
          [(k, "%.1e" % a, "%.1e" % b) for k, (a, b) in sorted(worst.items(), key=lambda kv: -kv[1][1])[:5]])
    # relative L2 2e-4 on every tensor (test_full_width_discriminator_backward_f32_matches_oracle_at_256's bar); single entries 1e-3:
    # the encoder's weight gradients sum 16384 pixels x 2304-4608 taps of f32 products behind a 15-layer f32 gradient chain
    assert all(a < 2e-4 and b < 1e-3 for a, b in worst.values()), {k: v for k, v in worst.items() if v[0] >= 2e-4 or v[1] >= 1e-3}


def _grads(m):
    return torch.cat([n.P.grad.clone() for n in m.networks()]).double()


def test_unet_bf16_step_at_full_width_close_to_f32(sg):
    """128x128, batch 8, ngf 64 (the 512-channel full-resolution layers on the halo kernels): the bf16 step is finite and close
    to the f32 step on the same parameters and inputs."""
    out = {}
    for dtype in ("f32", "bf16"):
        m, _ = _unet_case(sg, 64, 64, 8, 7, dtype=dtype)
        m.train_step()
        out[dtype] = (m.losses(), m.fake_A.numpy(), _grads(m))
        del m
        torch.cuda.empty_cache()
    (gl32, dl32), f32img, g32 = out["f32"]
    (gl16, dl16), bfimg, g16 = out["bf16"]
    assert all(np.isfinite([gl16, dl16])) and torch.isfinite(g16).all()
    d = np.abs(bfimg - f32img)
    cos = float((g16 @ g32) / (g16.norm() * g32.norm()))
    print(f"bf16 vs f32 U-Net step: losses {gl16:.5f}/{gl32:.5f} {dl16:.5f}/{dl32:.5f}, image max {d.max():.3e} mean {d.mean():.3e}, "
          f"gradient cosine {cos:.5f}")
    assert abs(gl16 - gl32) < 1e-2 * abs(gl32) and abs(dl16 - dl32) < 1e-2 * abs(dl32)
    assert d.max() < 0.1 and d.mean() < 1e-2
    assert cos > 0.95


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_unet_graph_replay_equals_eager_bitwise(sg, dtype):
    def run(graph):
        m = sg.sggan(sg.default_args(use_resnet=False, ngf=16, ndf=16, dtype=dtype, graph=graph))
        out = []
        for step in range(3):
            m.real_A, m.seg_A, m.mask_A = _rand_inputs(2, 128, 128, m.discriminator, 60 + step)
            m.train_step()
            out.append([t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.iterations, n.P.grad)]
                       + [m._loss.clone(), m.fake_A.tensor().clone()])
        return m, out
    _, eager = run(False)
    mg, graph = run(True)
    assert mg._program is not None
    for step, (a, b) in enumerate(zip(eager, graph)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (step, i)


def test_unet_checkpoint_resume_cli_and_architecture_tag(sg, tmp_path):
    from sggan_amd.main import main, parse_args, synthetic_batches
    argv = ["--generator", "unet", "--epoch", "2", "--batch_size", "1", "--img_height", "128", "--img_width", "128", "--ngf", "8",
            "--ndf", "8", "--dtype", "f32", "--steps_per_epoch", "2", "--checkpoint_dir", str(tmp_path / "ck"), "--dataset_dir", "unit",
            "--test_dir", str(tmp_path / "test"), "--log_dir", str(tmp_path / "logs")]
    # uninterrupted two epochs against one epoch, save, reload into a new object, second epoch
    a = parse_args(argv)
    m = sg.sggan(a)
    m.train(a, synthetic_batches(m, a), log=lambda s: None)
    ref = m.generator.P.flat.clone()
    a1 = parse_args(argv); a1.epoch, a1.checkpoint_dir = 1, str(tmp_path / "ck2")
    m1 = sg.sggan(a1)
    m1.train(a1, synthetic_batches(m1, a1), log=lambda s: None)
    assert torch.load(tmp_path / "ck2" / "unit" / "gen" / "cp-0000.ckpt")["G"]["arch"] == "unet"
    a2 = parse_args(argv); a2.epoch, a2.checkpoint_dir, a2.continue_train = 1, str(tmp_path / "ck2"), True
    m2 = sg.sggan(a2)
    second = synthetic_batches(m2, a2)
    m2.train(a2, lambda ep: second(1), log=lambda s: None)
    assert m2.generator.P.step_count == 4 and torch.equal(m2.generator.P.flat, ref)
    # a ResNet checkpoint into a U-Net model (and back) is refused by name
    r = parse_args(argv[2:]); r.n_blocks = 2
    mr = sg.sggan(r)
    assert mr.arch == "resnet"
    mr.save(str(tmp_path / "ckr"), 0)
    with pytest.raises(ValueError, match="resnet.*unet"):
        sg.sggan(parse_args(argv)).load(str(tmp_path / "ckr"))
    with pytest.raises(ValueError, match="unet.*resnet"):
        mr.load(str(tmp_path / "ck2"))
    # an untagged checkpoint is a ResNet checkpoint
    path = tmp_path / "ckr" / "unit" / "gen" / "cp-0000.ckpt"
    sd = torch.load(path); del sd["G"]["arch"]; torch.save(sd, path)
    assert mr.load(str(tmp_path / "ckr"))
    # the CLI: --phase test translates from the checkpoint, one --phase train epoch runs
    out = main(argv[:-6] + ["--checkpoint_dir", str(tmp_path / "ck"), "--test_dir", str(tmp_path / "test"), "--dataset_dir", "unit",
                            "--phase", "test"])
    assert len(out) == 2 and os.path.exists(tmp_path / "test" / "synthetic_000.png") and os.path.exists(tmp_path / "test" / "real_synthetic_001.png")
    hist = main(argv[:2] + ["--epoch", "1"] + argv[4:-6] + ["--checkpoint_dir", str(tmp_path / "ck3"), "--dataset_dir", "unit",
                                                           "--test_dir", str(tmp_path / "t3"), "--log_dir", str(tmp_path / "logs")])
    assert len(hist) == 1 and np.isfinite(hist[0]["Generator Loss"])
