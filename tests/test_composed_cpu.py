"""The composed float64 oracle (tests/composed_oracle.py) checked without a GPU: with every option neutral it is the
plain U-Net steps' oracle, with one option on it is that option's own oracle (both share the ops they compare: these guard the
wiring of the arguments, and agree exactly), all-on it agrees with a second, independent statement written in torch float64
autograd, and at the fixed seeds of tests/test_gpu_composed.py the oracle alone stays under the ambiguity caps the GPU tests assert."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sggan_oracle as O
from oracle import torch_restatement as T
from tests import composed_oracle as CO
from tests import diffaug_oracle as DA
from tests import dropout_oracle as DO
from tests import spectral_oracle as S
from tests import ssim_loss_oracle as SL
from tests import unet_cycle_oracle as UC
from tests import unet_oracle as UO

H = W = 128                     # the smallest size the U-Net and the discriminator's 1 x 1 head accept
BOUND, TWIN_BOUND = 1e-12, 1e-9


def _err(got, exp):
    return float(np.abs(np.asarray(got, np.float64) - exp).max() / max(np.abs(exp).max(), 1e-300))


def _same_grads(got, exp, bound, what):
    assert set(got) == set(exp), what
    # (a bias in front of an unmasked instance norm has gradient 0: float64 leaves rounding noise of ~1e-16 there in both statements)
    worst = max(((_err(got[k], exp[k]), k) for k in exp if np.abs(exp[k]).max() >= 1e-9), default=(0.0, None))
    zero = [k for k in exp if np.abs(exp[k]).max() < 1e-9 and np.abs(got[k]).max() >= 1e-9]
    print(f"{what}: worst tensor {worst[1]} at {worst[0]:.2e} of its largest entry")
    assert worst[0] <= bound and not zero, (what, worst, zero)


def _same_step(got, exp, bound, what, keys):
    for a, b in keys["losses"]:
        assert abs(got[a] - exp[b]) <= bound * abs(exp[b]), (what, a, got[a], exp[b])
    for a, b in keys["grads"]:
        ga, gb = got, exp
        for k in a:
            ga = ga[k]
        for k in b:
            gb = gb[k]
        _same_grads(ga, gb, bound, f"{what} {'.'.join(a)}")


REF_KEYS = {"losses": (("gen_loss", "gen_loss"), ("disc_loss", "disc_loss")), "grads": ((("gG",), ("gG",)), (("gD",), ("gD",)))}
CYC_KEYS = {"losses": (("g_loss", "g_loss"), ("d_loss", "d_loss")),
            "grads": tuple((("grads", n), ("grads", n)) for n in ("Gab", "Gba", "Da", "Db"))}


@pytest.fixture(scope="module")
def small():
    """1 x 128 x 128, ndf 4: U-Net (ngf 2) and ResNet (ngf 4, one block) generators, instance-norm and spectral discriminators."""
    rng = np.random.default_rng(7)
    out = {"unet": CO.case_params(rng, True, 2, 4, spectral=False), "resnet": CO.case_params(rng, True, 4, 4, spectral=False, generator="resnet"),
           "sn": CO.case_params(rng, True, 4, 4, spectral=True, generator="resnet")}
    out["A"], out["B"] = CO.case_inputs(rng, 1), CO.case_inputs(rng, 1)
    shapes = S.discriminator_param_shapes(df_dim=4)
    out["Ua"], out["Ub"] = S.init_u(shapes, rng), S.init_u(shapes, rng)
    return out


# ---- 1. neutral options, then one at a time ---------------------------------------------------------------------------------------
def test_neutral_options_give_the_plain_unet_steps(small):
    P, (rA, sA, mA), (rB, sB, mB) = small["unet"], small["A"], small["B"]
    got = CO.reference_step(P["Gab"], P["Da"], None, rA, sA, mA)
    _same_step(got, UO.train_step(P["Gab"], P["Da"], rA, sA, mA), BOUND, "reference", REF_KEYS)
    got = CO.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], None, None, rA, rB, sA, sB, mA, mB)
    exp = UC.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], rA, rB, sA, sB, mA, mB)
    _same_step(got, exp, BOUND, "cycle", CYC_KEYS)
    for k in ("fake_A", "fake_B", "cyc_A", "cyc_B"):
        assert _err(got[k], exp[k]) <= BOUND


def test_spectral_alone_is_the_spectral_oracle(small):
    P, (rA, sA, mA), (rB, sB, mB) = small["sn"], small["A"], small["B"]
    kw = dict(generator="resnet", n_blocks=1)
    got = CO.reference_step(P["Gab"], P["Da"], small["Ua"], rA, sA, mA, **kw)
    exp = S.train_step(P["Gab"], P["Da"], small["Ua"], rA, sA, mA, n_blocks=1)
    _same_step(got, exp, BOUND, "reference", REF_KEYS)
    assert all(np.array_equal(got["U"][n], exp["U"][n]) for n in S.LAYERS)
    got = CO.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], small["Ua"], small["Ub"], rA, rB, sA, sB, mA, mB, **kw)
    exp = S.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], small["Ua"], small["Ub"], rA, rB, sA, sB, mA, mB, n_blocks=1)
    _same_step(got, exp, BOUND, "cycle", CYC_KEYS)
    assert all(np.array_equal(got[u][n], exp[u][n]) for u in ("Ua", "Ub") for n in S.LAYERS)


def test_ssim_alone_is_the_ssim_oracle(small):
    P, (rA, sA, mA), (rB, sB, mB) = small["resnet"], small["A"], small["B"]
    kw = dict(generator="resnet", n_blocks=1, ssim_lambda=5.0, data_range=0.8)
    got = CO.reference_step(P["Gab"], P["Da"], None, rA, sA, mA, **kw)
    _same_step(got, SL.train_step(P["Gab"], P["Da"], rA, sA, mA, 5.0, 0.8, n_blocks=1), BOUND, "reference", REF_KEYS)
    got = CO.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], None, None, rA, rB, sA, sB, mA, mB, **kw)
    exp = SL.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], rA, rB, sA, sB, mA, mB, 5.0, 0.8, n_blocks=1)
    _same_step(got, exp, BOUND, "cycle", CYC_KEYS)


def test_diffaug_alone_is_the_diffaug_oracle(small):
    P, (rA, sA, mA) = small["resnet"], small["A"]
    rows = CO.reference_rows(3, 1, H, W)
    got = CO.reference_step(P["Gab"], P["Da"], None, rA, sA, mA, rows=rows, generator="resnet", n_blocks=1)
    _same_step(got, DA.train_step(P["Gab"], P["Da"], rA, sA, mA, rows, n_blocks=1), BOUND, "reference", REF_KEYS)
    assert not np.array_equal(rows[0], DA.NEUTRAL) and not np.array_equal(rows[0], rows[1])
    # neutral rows are the step without the option
    plain = CO.reference_step(P["Gab"], P["Da"], None, rA, sA, mA, generator="resnet", n_blocks=1)
    off = CO.reference_step(P["Gab"], P["Da"], None, rA, sA, mA, rows=np.tile(DA.NEUTRAL, (2, 1)), generator="resnet", n_blocks=1)
    _same_step(off, plain, BOUND, "neutral rows", REF_KEYS)


def test_dropout_op_is_where_the_torch_statement_puts_it():
    """The masked generator alone, 2 x 16 x 16, ngf 2: output and every gradient against dropout_oracle.torch_generator_unet; a
    mask of ones at rate 0 is the inference-mode network."""
    rng = np.random.default_rng(5)
    P = {k: CO.f32(v) for k, v in O.init_params(UO.unet_param_shapes(2, 3, 3), rng, 0.1).items()}
    x, dy = rng.uniform(0, 1, (2, 16, 16, 3)), rng.standard_normal((2, 16, 16, 3))
    masks = CO.generator_masks(5, 19, 1, 2, 16, 16, 16, sample_offset=3)
    assert all(0.3 < m.mean() < 0.7 for m in masks)

    def taped(masks, rate):
        tape = O.Tape()
        V, vx = {k: O.Var(v, k) for k, v in P.items()}, O.Var(x)
        y = CO.generator_unet(tape, V, vx, masks, rate)
        tape.backward([(y, dy)])
        return y.v, {k: v.g for k, v in V.items()}, vx.g
    y, g, dx = taped(masks, 0.5)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in P.items()}
    tx = torch.tensor(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ye = DO.torch_generator_unet(tp, tx, [torch.tensor(m).permute(0, 3, 1, 2) for m in masks], 0.5)
    (ye * torch.tensor(dy).permute(0, 3, 1, 2)).sum().backward()
    assert _err(y, ye.detach().permute(0, 2, 3, 1).numpy()) <= TWIN_BOUND and _err(dx, tx.grad.permute(0, 2, 3, 1).numpy()) <= TWIN_BOUND
    _same_grads(g, {k: v.grad.numpy() for k, v in tp.items()}, TWIN_BOUND, "masked generator")
    assert all(np.abs(g[k]).max() > 0 for k in ("d1_b", "d2_b", "d3_b"))            # (a bias in front of a masked norm counts)
    y0, g0, dx0 = taped(None, 0.5)
    y1, g1, dx1 = taped([np.ones_like(m) for m in masks], 0.0)
    assert _err(y1, y0) <= BOUND and _err(dx1, dx0) <= BOUND
    _same_grads({k: v for k, v in g1.items() if not k.endswith("_b")}, {k: v for k, v in g0.items() if not k.endswith("_b")}, BOUND, "ones")


# ---- 2. a second statement of the all-on reference step -------------------------------------------------------------------------
def _torch_diffaug(x, rows):
    """diffaug_oracle.forward on an NCHW float64 tensor (for fixed rows the transform is affine; autograd takes its adjoint)."""
    out = []
    for n in range(x.shape[0]):
        b, s, c = (float(v) for v in rows[n, :3])
        x1 = x[n] + b
        x2 = x1 + (s - 1.0) * (x1 - x1.mean(0, keepdim=True))
        x3 = x2 + (c - 1.0) * (x2 - (b + x[n].mean()))
        keep = torch.tensor(~DA._inside(rows[n], x.shape[2], x.shape[3]))
        out.append(x3 * keep)
    return torch.stack(out)


def _torch_spectral_discriminator(P, U1, V, x, mask, leak=0.3):
    """The discriminator without its norms on W / sigma, sigma = v^T M u with u and v constants."""
    h = x
    for name, stride, pad in (("h0", 2, "SAME"), ("h1", 2, "SAME"), ("h2", 2, "SAME"), ("h3", 1, "SAME"),
                              ("h31", 2, "VALID"), ("h32", 2, "VALID"), ("h33", 1, "VALID"), ("h4", 1, "SAME")):
        w = P[name + "_w"]
        sigma = torch.clamp(torch.tensor(V[name]) @ w.reshape(-1, w.shape[-1]) @ torch.tensor(U1[name]), min=S.EPS)
        h = T.conv2d(h, w / sigma, P[name + "_b"], stride, pad)
        if name != "h4":
            h = F.leaky_relu(h, leak)
    return (h * mask).sum(1, keepdim=True)


def torch_reference_step(PG, PD, U, real_A, seg_A, mask_A, masks, rows, ssim_lambda, data_range, rate=0.5, l1_lambda=100.0):
    N = real_A.shape[0]
    to = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64).permute(0, 3, 1, 2).contiguous()
    leaf = lambda P: {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in P.items()}
    tG, tD = leaf(PG), leaf(PD)
    U1, V, _ = S.iterate(PD, U)
    fake = DO.torch_generator_unet(tG, to(real_A), [to(m) for m in masks], rate)
    seg, mask = to(seg_A), to(mask_A)
    da_real = _torch_spectral_discriminator(tD, U1, V, _torch_diffaug(seg, rows[:N]), mask)
    da_fake = _torch_spectral_discriminator(tD, U1, V, _torch_diffaug(fake, rows[N:]), mask)
    bce = lambda x, z: F.binary_cross_entropy_with_logits(x, torch.full_like(x, z))
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    gen_loss = bce(da_fake, 1.0) + l1_lambda * (seg - fake).abs().mean() + ssim_lambda * SL.loss_torch(nhwc(seg), nhwc(fake), data_range)
    disc_loss = bce(da_real, 1.0) + bce(da_fake, 0.0)
    gG = torch.autograd.grad(gen_loss, list(tG.values()), retain_graph=True)
    gD = torch.autograd.grad(disc_loss, list(tD.values()))
    return {"gen_loss": gen_loss.item(), "disc_loss": disc_loss.item(), "gG": {k: g.numpy() for k, g in zip(tG, gG)},
            "gD": {k: g.numpy() for k, g in zip(tD, gD)}, "fake_A": nhwc(fake.detach()).numpy()}


def test_all_on_reference_step_agrees_with_its_torch_autograd_statement():
    """1 x 128 x 128, ngf 4, ndf 4, every option on: the tape against torch float64 autograd at 1e-9 of each tensor's largest
    entry (tests/test_unet_cycle_cpu.py's bound for the same kind of twin)."""
    rng = np.random.default_rng(11)
    P = CO.case_params(rng, False, 4, 4)
    real, seg, mask = CO.case_inputs(rng, 1)
    U = S.init_u(S.discriminator_param_shapes(df_dim=4), rng)
    masks, rows = CO.generator_masks(1, 19, 0, 1, H, W, 32), CO.reference_rows(1, 1, H, W)
    got = CO.reference_step(P["Gab"], P["Da"], U, real, seg, mask, masks=masks, rows=rows, ssim_lambda=5.0, data_range=1.0)
    exp = torch_reference_step(P["Gab"], P["Da"], U, real, seg, mask, masks, rows, 5.0, 1.0)
    _same_step(got, exp, TWIN_BOUND, "all-on reference", REF_KEYS)
    assert _err(got["fake_A"], exp["fake_A"]) <= TWIN_BOUND
    assert all(np.abs(got["gG"][k]).max() > 0 for k in ("d1_b", "d2_b", "d3_b")) and all(np.abs(g).max() > 0 for g in got["gD"].values())
    # ... and the update chain's transform of dL / d(W / sigma) is the tape's gradient with respect to W
    sp = ({k: v for k, v in P["Da"].items()}, got["U"], got["V"], got["sigma"])
    g = dict(got["gD"], **{n + "_w": got["gD_scaled"][n] for n in S.LAYERS})
    z = {k: np.zeros_like(v) for k, v in P["Da"].items()}
    *_, info = CO.network_update(P["Da"], g, z, z, 0, lr=1e-3, spectral=sp)
    _same_grads(info["g"], got["gD"], BOUND, "spectral transform in the update chain")


# ---- 3. the update chain ---------------------------------------------------------------------------------------------------------
def test_update_chain_order_clip_rate_average_and_skip():
    from sggan_amd import kernels as K
    from tests import ema_oracle as E
    rng = np.random.default_rng(3)
    th = {"a": rng.standard_normal((3, 4)), "b": rng.standard_normal(5)}
    g = {"a": rng.standard_normal((3, 4)), "b": rng.standard_normal(5)}
    z = {k: np.zeros_like(v) for k, v in th.items()}
    norm = float(np.sqrt(sum((v ** 2).sum() for v in g.values())))
    t1, m1, v1, it, ema, info = CO.network_update(th, g, z, z, 2, th, lr=1e-3, max_norm=norm / 2, sched=(1, 1, 4), ema_decay=0.999)
    assert it == 3 and not info["skip"] and abs(info["norm"] - norm) < 1e-12 * norm and info["clip"] == float(np.float32(np.float32(norm / 2) / norm))
    assert info["lr"] == float(K.scheduled_lr(1e-3, 2, 1, 1, 4)) == float(np.float32(float(np.float32(1e-3)) * 2.0 / 3.0))
    flat = lambda d: np.concatenate([d[k].reshape(-1) for k in ("a", "b")])
    e = K.guarded_update(flat(th), flat(g), flat(z), flat(z), 2, 1e-3, 0.5, 0.999, 1e-7, 1.0, norm / 2, (1, 1, 4))
    assert np.array_equal(flat(t1), e[0]) and np.array_equal(flat(m1), e[1]) and np.array_equal(flat(v1), e[2])
    assert np.array_equal(flat(ema), E.ema_step(flat(th), e[0], 0.999, 3))          # the average moves to the NEW parameters at t = 3
    bad = dict(g, b=np.where(np.arange(5) == 2, np.nan, g["b"]))
    t2, m2, v2, it2, ema2, info2 = CO.network_update(th, bad, z, z, 2, th, lr=1e-3, max_norm=norm / 2, sched=(1, 1, 4), ema_decay=0.999)
    assert info2["skip"] and it2 == 2 and all(np.array_equal(t2[k], th[k]) and np.array_equal(ema2[k], th[k]) for k in th)


# ---- 4. the ambiguity caps of the GPU tests' seeds, on the oracle alone ------------------------------------------------------------
def test_reference_case_seed_stays_under_the_kink_cap():
    rng = np.random.default_rng(CO.REFERENCE_CASE_SEED)
    P = CO.case_params(rng, False)
    real, seg, mask = CO.case_inputs(rng)
    U = S.init_u(S.discriminator_param_shapes(df_dim=8), rng)
    pol = O.KinkPolicy(1e-4)
    O.KINKS = pol
    try:
        CO.reference_step(P["Gab"], P["Da"], U, real, seg, mask, masks=CO.generator_masks(0, CO.SEED, 0, 2, H, W, 64),
                          rows=CO.reference_rows(0, 2, H, W), ssim_lambda=CO.SSIM_LAMBDA)
    finally:
        O.KINKS = None
    print(f"reference case: {pol.ambiguous} of {pol.elements} pre-activations within 1e-4 of a kink")
    assert pol.calls == 10 + 2 * 7 and pol.ambiguous < 1e-3 * pol.elements


def test_cycle_case_seed_stays_under_the_kink_and_sign_caps():
    rng = np.random.default_rng(CO.CYCLE_CASE_SEED)
    P = CO.case_params(rng, True)
    (rA, sA, mA), (rB, sB, mB) = CO.case_inputs(rng), CO.case_inputs(rng)
    shapes = S.discriminator_param_shapes(df_dim=8)
    Ua, Ub = S.init_u(shapes, rng), S.init_u(shapes, rng)
    pol = O.KinkPolicy(1e-4)
    O.KINKS = pol
    try:
        r = CO.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], Ua, Ub, rA, rB, sA, sB, mA, mB, masks=CO.cycle_masks(0, 0, 2, H, W, 64),
                          rows=CO.cycle_rows(0, 0, 2, H, W), ssim_lambda=CO.SSIM_LAMBDA)
    finally:
        O.KINKS = None
    elements, ambiguous = CO.sign_counts(r, rA, rB, sA, sB)
    print(f"cycle case: {pol.ambiguous} of {pol.elements} pre-activations within 1e-4 of a kink, {ambiguous} of {elements} sign() "
          "arguments within 1e-4 of zero")
    assert pol.calls == 4 * 10 + 4 * 7 and pol.ambiguous < 1e-3 * pol.elements
    assert elements > 0 and ambiguous < 1e-3 * elements


# ---- 5. the flags ----------------------------------------------------------------------------------------------------------------
def test_all_flags_together_reach_the_namespace():
    from sggan_amd.main import parse_args
    a = parse_args(["--generator", "unet", "--cycle", "--ssim_lambda", "5", "--ssim_data_range", "0.8", "--diffaug", "color,cutout",
                    "--d_norm", "spectral", "--dropout", "--ema_decay", "0.999", "--lr_decay", "--clip_grad_norm", "2.5",
                    "--skip_nonfinite"])
    assert (a.use_resnet, a.cycle, a.ssim_lambda, a.ssim_data_range, a.diffaug, a.d_norm, a.dropout, a.ema_decay, a.lr_decay,
            a.clip_grad_norm, a.skip_nonfinite) == (False, True, 5.0, 0.8, "color,cutout", "spectral", 0.5, 0.999, True, 2.5, True)
