"""Cycle mode with the U-Net generators on the MI355X path: the lockstep skip-before-activation norm (sgg_instnorm_*_skip_pair)
bit for bit against the single-network form and against float64, the paired step against the kink-aware float64 oracle
(tests/unet_cycle_oracle.py), paired against one-network-at-a-time, HIP-graph replay, the CLI / checkpoints / pool / data
parallel combinations and the bf16 step at full width."""
import os
import socket
import warnings

import numpy as np
import pytest
import torch

from oracle import sggan_oracle as O
from tests import unet_cycle_oracle as UC
from tests import unet_oracle as U
from tests.test_gpu_exact import dev, store
from tests.test_gpu_step import _l2, _rand_inputs, rel
from tests.test_gpu_unet import _skip_norm_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "city_small")


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


# ----------------------------------------------------------------------------- 1. the lockstep skip norm
# (N, nsplit, H, W, C, dtype).  The kernels walk (pixel row, channel vector) pairs: a block has 256 / lanes pixel rows in flight,
# lanes = min(C / VEC, 256) channel vectors (VEC 8 for bf16, 4 for f32); statistics chunks and apply blocks hold 64 pixels at
# these sizes.  7x9 = 63 pixels at C = 8: one chunk, many rows per block, only the tail loops.  7x29 = 203 pixels: four chunks,
# the last with 11 pixels.  C = 24: lanes = 3 / 6 (256 % lanes != 0: idle threads).  C = 128: 16 / 8 rows in flight, so the 64
# pixels of a block reach the 4-pixel (apply) and 2-pixel (backward statistics) unrolled trips and their tails.  C = 1032 in
# f32: 258 channel vectors, the second trip of the `cvb += 256` sweep.
SKIP_CASES = [(2, 1, 7, 9, 8, torch.bfloat16), (2, 1, 7, 9, 8, torch.float32),
              (3, 1, 7, 29, 24, torch.bfloat16), (3, 1, 7, 29, 24, torch.float32),
              (3, 2, 7, 29, 128, torch.bfloat16), (3, 2, 7, 29, 128, torch.float32),
              (2, 1, 7, 9, 1032, torch.float32)]


@pytest.mark.parametrize("act", ["relu", "lrelu", "none"])
@pytest.mark.parametrize("case", SKIP_CASES, ids=lambda c: f"N{c[0]}s{c[1]}_{c[2]}x{c[3]}x{c[4]}_{str(c[5]).split('.')[-1]}")
def test_pair_skip_norm_equals_single_form_bitwise_and_float64(sg, case, act):
    """sgg_instnorm_fwd_skip_pair / _partial_pair / sgg_instnorm_bwd_skip_pair on a stacked tensor against sgg_instnorm_*_skip on
    each half with that half's own gamma / beta: every output bit for bit (torch.equal), with accumulate 0 and 1.  And against the
    float64 formula at the bars of test_skip_before_activation_norm_matches_float64 (f32 1e-5 forward / 2e-5 backward, bf16
    2e-2 / 3e-2), so that agreeing with a wrong single form does not pass."""
    from sggan_amd import _abi as A
    from sggan_amd import kernels as K
    N, ns, H, W, C, dtype = case
    code, leak = {"relu": (A.ACT_RELU, 0.0), "lrelu": (A.ACT_LRELU, float(np.float32(0.3))), "none": (A.ACT_NONE, 0.0)}[act]
    rng = np.random.default_rng(1000 * C + 10 * N + ns)
    rnd = lambda a=1.0, b=0.0: store(rng.standard_normal((N, H, W, C)) * a + b, dtype)
    x, skip, dy = rnd(3.0, 1.0), rnd(), rnd()
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    # distinct parameters per half: a mix-up of the two sets shows in every output
    gam = [f32(1 + 0.2 * rng.standard_normal(C)), f32(-0.7 + 0.2 * rng.standard_normal(C))]
    bet = [f32(0.2 * rng.standard_normal(C)), f32(0.5 + 0.2 * rng.standard_normal(C))]
    tx, ts, tdy = dev(x, dtype), dev(skip, dtype), dev(dy, dtype)
    tg, tb = [dev(g) for g in gam], [dev(b) for b in bet]
    halves = (slice(0, ns), slice(ns, N))

    y, stats = K.instnorm_fwd_skip_pair(tx, tg[0], tb[0], tg[1], tb[1], ns, ts, 1e-3, code, leak)
    xs = tx.to(torch.float64)                                 # host-made (sum, sumsq) rows: one chunk per image
    part = torch.stack([xs.sum((1, 2)), (xs * xs).sum((1, 2))], -1)[:, None].to(torch.float32).contiguous()
    y2, stats2 = K.instnorm_fwd_skip_pair(tx, tg[0], tb[0], tg[1], tb[1], ns, ts, 1e-3, code, leak, partial=part)
    ftol, btol = (1e-5, 2e-5) if dtype == torch.float32 else (2e-2, 3e-2)
    exp = []
    for h, sl in enumerate(halves):
        xh, sh = tx[sl].contiguous(), ts[sl].contiguous()
        ys, st = K.instnorm_fwd_skip(xh, tg[h], tb[h], sh, 1e-3, code, leak)
        assert torch.equal(y[sl], ys) and torch.equal(stats[sl], st), ("forward", h)
        ys2, st2 = K.instnorm_fwd_skip(xh, tg[h], tb[h], sh, 1e-3, code, leak, partial=part[sl].contiguous())
        assert torch.equal(y2[sl], ys2) and torch.equal(stats2[sl], st2), ("forward from partial sums", h)
        pos = (ys > 0).cpu().numpy() if act != "none" else np.ones(ys.shape, bool)
        e = _skip_norm_oracle(x[sl], gam[h], bet[h], skip[sl], dy[sl], pos, leak if act != "none" else 1.0)
        if act != "none":
            assert not (pos != (e[0] > 0))[np.abs(e[0]) > 1e-4].any()      # the kernel's branch is float64's outside the rounding band
        assert rel(ys.float().cpu().numpy(), e[1]) < ftol and rel(ys2.float().cpu().numpy(), e[1]) < ftol, ("float64 forward", h)
        exp.append(e)

    for accumulate in (0, 1):
        init = (0.5, -0.5) if accumulate else (7.0, 7.0)      # (accumulate 0 overwrites whatever is there)
        mk = lambda v: torch.full((C,), v, device="cuda")
        dg, db = [mk(init[0]), mk(init[0])], [mk(init[1]), mk(init[1])]
        dx, dskip = K.instnorm_bwd_skip_pair(tdy, y, tx, tg[0], tb[0], tg[1], tb[1], ns, stats, dg[0], db[0], dg[1], db[1],
                                             accumulate=bool(accumulate), act=code, leak=leak)
        for h, sl in enumerate(halves):
            dgs, dbs = mk(init[0]), mk(init[1])
            dxs, dss = K.instnorm_bwd_skip(tdy[sl].contiguous(), y[sl].contiguous(), tx[sl].contiguous(), tg[h], tb[h],
                                           stats[sl].contiguous(), dgs, dbs, accumulate=bool(accumulate), act=code, leak=leak)
            assert torch.equal(dx[sl], dxs) and torch.equal(dskip[sl], dss), ("backward", accumulate, h)
            assert torch.equal(dg[h], dgs) and torch.equal(db[h], dbs), ("parameter gradients", accumulate, h)
            z, ye, dz, dxe, dge, dbe = exp[h]
            assert np.array_equal(dss.float().cpu().numpy(), store(dz, dtype))        # dy * act'(y): one multiply, one rounding
            assert rel(dxs.float().cpu().numpy(), dxe) < btol
            base = init if accumulate else (0.0, 0.0)
            assert rel(dgs.cpu().numpy() - base[0], dge) < btol and rel(dbs.cpu().numpy() - base[1], dbe) < btol


def test_pair_skip_norm_argument_checks(sg):
    """Argument checks follow the other pair forms: a split outside (0, N) or a missing second set is SGG_EINVAL; tanh is
    SGG_EUNSUPPORTED, as in the single forms."""
    from sggan_amd import _abi as A
    from sggan_amd import kernels as K
    x = torch.randn(2, 8, 8, 8, device="cuda")
    g = torch.ones(8, device="cuda")
    for bad in (0, 2):
        with pytest.raises(AssertionError):
            K.instnorm_fwd_skip_pair(x, g, g, g, g, bad, x)
    y, stats = K.instnorm_fwd_skip_pair(x, g, g, g, g, 1, x, act=A.ACT_RELU)
    ws = K.workspace(int(A.lib().sgg_instnorm_workspace(2, 64, 8)), x.device)
    p = K._p
    fwd = lambda ns, g2, act: A.lib().sgg_instnorm_fwd_skip_pair(p(x), p(g), p(g), g2, p(g), ns, p(x), p(y), p(stats), 2, 64, 8, 1e-3, act, 0.0,
                                                                   A.SGG_F32, p(ws), ws.numel(), K._s())
    assert fwd(1, p(g), A.ACT_RELU) == A.OK
    assert fwd(0, p(g), A.ACT_RELU) == A.EINVAL and fwd(2, p(g), A.ACT_RELU) == A.EINVAL and fwd(1, None, A.ACT_RELU) == A.EINVAL
    assert fwd(1, p(g), A.ACT_TANH) == A.EUNSUPPORTED
    dx, dskip, dg = torch.empty_like(x), torch.empty_like(x), torch.zeros(8, device="cuda")
    bwd = lambda ns, dg2, act: A.lib().sgg_instnorm_bwd_skip_pair(p(x), p(y), p(x), p(g), p(g), p(g), p(g), ns, p(stats), p(dx), p(dskip),
                                                                    p(dg), p(dg), dg2, p(dg), 2, 64, 8, 8, 0, act, 0.0, A.SGG_F32, p(ws), ws.numel(), K._s())
    assert bwd(1, p(dg), A.ACT_RELU) == A.OK
    assert bwd(2, p(dg), A.ACT_RELU) == A.EINVAL and bwd(1, None, A.ACT_RELU) == A.EINVAL and bwd(1, p(dg), A.ACT_TANH) == A.EUNSUPPORTED
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 2. the step against float64
def _f32(a):
    return a.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("d_quad", [False, True], ids=["two_passes", "d_quad"])
@pytest.mark.parametrize("use_lsgan", [True, False], ids=["lsgan", "sce"])
def test_unet_cycle_step_f32_matches_kink_aware_oracle(sg, use_lsgan, d_quad):
    """One paired f32 cycle step with U-Net generators (1x128x128, ngf 8, ndf 8, the 4x4 mask grid of the (1,1) broadcast rule)
    against tests/unet_cycle_oracle.cycle_step evaluated kink-aware (oracle.KinkPolicy at 1e-4, branches read from the step's
    saved records).  Bars: losses 2e-5; fakes 1e-4, cycle images 2e-4; every gradient tensor 2e-4 relative L2 and 1e-3 worst
    entry over largest entry (test_unet_reference_step_f32_matches_kink_aware_oracle's); post-Adam parameters 2e-5 on entries
    whose gradient is above 1e-2 of the tensor's largest (Adam's first step is -lr * g / (|g| + 1e-7), i.e. -lr * sign(g): with
    every entry held to 1e-3 of the largest, entries ten times that size cannot change sign; smaller ones may)."""
    ngf = ndf = 8
    N, H, W = 1, 128, 128
    rng = np.random.default_rng(31)
    gs, ds = U.unet_param_shapes(ngf, 3, 3), O.discriminator_param_shapes(df_dim=ndf)
    P = {n: {k: _f32(v) for k, v in O.init_params(sh, rng, 0.1).items()} for n, sh in (("Gab", gs), ("Gba", gs), ("Da", ds), ("Db", ds))}
    real_A, real_B = _f32(rng.uniform(0, 1, (N, H, W, 3))), _f32(rng.uniform(0, 1, (N, H, W, 3)))
    pal = rng.integers(0, 256, (8, 3)) / 255.0
    blocks = lambda: _f32(pal[np.repeat(np.repeat(rng.integers(0, 8, (N, H // 32, W // 32)), 32, 1), 32, 2)])
    seg_A, seg_B = blocks(), blocks()
    m = sg.sggan(sg.default_args(use_resnet=False, ngf=ngf, ndf=ndf, dtype="f32", cycle=True, use_lsgan=use_lsgan, keep_tapes=True,
                                 d_quad=d_quad, paired=True))
    assert m.discriminator.out_hw(H, W) == (1, 1)             # one logit per class, broadcast over the mask grid
    mk = lambda: np.stack([O.one_hot(i, 34) for i in rng.integers(0, 34, (N, 4, 4))]).astype(np.float64)
    mask_A, mask_B = mk(), mk()
    assert m.arch == "unet" and m.paired and type(m.generator_BA).__name__ == "GeneratorUNet"
    nets = {"Gab": m.generator, "Gba": m.generator_BA, "Da": m.discriminator, "Db": m.discriminator_B}
    for n, net in nets.items():
        net.P.load(P[n])
    m.real_A, m.real_B, m.seg_A, m.seg_B, m.mask_A, m.mask_B = real_A, real_B, seg_A, seg_B, mask_A, mask_B
    m.train_step()
    gl, dl = m.losses()
    assert type(m._pairs[0]).__name__ == "GeneratorUNetPair" and (m.tapes["D_quad"] is not None) == d_quad
    branches = UC.unet_cycle_step_branches(m)
    pol = O.KinkPolicy(1e-4, branches)
    O.KINKS = pol
    try:
        r = UC.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], real_A, real_B, seg_A, seg_B, mask_A, mask_B, use_lsgan=use_lsgan)
    finally:
        O.KINKS = None
    print(f"kink-aware U-Net cycle oracle [d_quad={d_quad}]: {pol.elements} activations, {pol.ambiguous} within 1e-4 of a kink, "
          f"{pol.overridden} overridden, {pol.disagree_outside} disagreements outside the band")
    print(f"losses: g {gl:.8f} / {r['g_loss']:.8f}  d {dl:.8f} / {r['d_loss']:.8f}")
    imgs = {k: rel(getattr(m, k).numpy(), r[k]) for k in ("fake_A", "fake_B", "cyc_A", "cyc_B")}
    print("images (worst entry / largest):", {k: "%.1e" % v for k, v in imgs.items()})
    worst = {}
    for n, net in nets.items():
        got = net.P.export(net.P.grad)
        for k, e in r["grads"][n].items():
            if np.abs(e).max() < 1e-9:            # biases in front of a norm; at 128x128 everything in front of D's 1x1 h33 norm
                assert np.abs(got[k]).max() < 1e-6, (n, k)
                continue
            worst[(n, k)] = (_l2(got[k], e), rel(got[k], e))
    top = sorted(worst.items(), key=lambda kv: -max(kv[1][0], kv[1][1] / 5))[:5]
    print("largest gradient errors (relative L2, worst entry / largest entry):", [(k, "%.1e" % v[0], "%.1e" % v[1]) for k, v in top])
    assert pol.calls == len(branches) and pol.disagree_outside == 0
    assert abs(gl - r["g_loss"]) < 2e-5 * abs(r["g_loss"]) and abs(dl - r["d_loss"]) < 2e-5 * abs(r["d_loss"])
    assert imgs["fake_A"] < 1e-4 and imgs["fake_B"] < 1e-4 and imgs["cyc_A"] < 2e-4 and imgs["cyc_B"] < 2e-4
    assert len(worst) >= 2 * 47 + 2 * 3
    bad = {k: v for k, v in worst.items() if not (v[0] < 2e-4 and v[1] < 1e-3)}
    assert not bad, bad
    for n, net in nets.items():
        new = net.P.export()
        for k, e in r["params"][n].items():
            ge = r["grads"][n][k]
            if np.abs(ge).max() < 1e-9:
                continue
            sig = np.abs(ge) > 1e-2 * np.abs(ge).max()
            assert np.abs(new[k] - e)[sig].max() < 2e-5, (n, "post-Adam", k)


# ----------------------------------------------------------------------------- 3. paired == one network at a time
def _cycle_inputs(m, N, H, W, seed):
    m.real_A, m.seg_A, m.mask_A = _rand_inputs(N, H, W, m.discriminator, seed)
    m.real_B, m.seg_B, m.mask_B = _rand_inputs(N, H, W, m.discriminator, seed + 1)


def _state(m):
    return ([t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.grad)] +
            [m._loss.clone(), m.fake_A.tensor(), m.fake_B.tensor(), m.cyc_A.tensor(), m.cyc_B.tensor()])


@pytest.mark.parametrize("cfg", [("f32", 16, 2), ("bf16", 16, 2), ("bf16", 64, 1)], ids=["f32_small", "bf16_small", "bf16_full_width_halo_paths"])
def test_unet_paired_cycle_step_equals_one_network_at_a_time(sg, cfg):
    """GeneratorUNetPair (stacked batches, one launch per pair for every norm -- the skip norms included -- and for the 3x3 halo
    GEMMs) against the one-network-at-a-time sequencing with GeneratorUNet, d_quad off: losses, the four images and every data
    gradient bitwise equal.  Parameter / slot / gradient buffers may differ by f32 summation order where two networks' weight
    gradients share a launch: held to 1e-5 of their norm (test_paired_cycle_step_is_bit_identical_to_one_network_at_a_time's
    rule).  ngf 64 at 128x128: the 512-channel full-resolution layers on the halo kernels (W % 128 == 0)."""
    dtype, width, N = cfg
    out = []
    for paired in (False, True):
        m = sg.sggan(sg.default_args(use_resnet=False, ngf=width, ndf=width, dtype=dtype, cycle=True, paired=paired, d_quad=False))
        _cycle_inputs(m, N, 128, 128, 61)
        m.train_step()
        assert (getattr(m, "_pairs", None) is not None) == paired
        out.append(_state(m))
        del m
    names = [f"net{k}.{what}" for k in range(4) for what in ("flat", "m", "v", "grad")] + ["loss", "fake_A", "fake_B", "cyc_A", "cyc_B"]
    inexact = 0
    for name, a, b in zip(names, *out):
        assert torch.isfinite(a.float()).all(), name
        if torch.equal(a, b):
            continue
        assert name.startswith("net"), name       # only parameter / slot / gradient buffers may differ, and only by summation order
        d = float((a.double() - b.double()).norm() / b.double().norm())
        assert d < 1e-5, (name, d)
        inexact += 1
    print("tensors equal up to f32 summation order only:", inexact)


# ----------------------------------------------------------------------------- 4. graph replay
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_unet_cycle_graph_replay_equals_eager_bitwise(sg, dtype):
    def run(graph):
        m = sg.sggan(sg.default_args(use_resnet=False, ngf=16, ndf=16, dtype=dtype, cycle=True, graph=graph, paired=True))
        out = []
        for step in range(3):
            _cycle_inputs(m, 2, 128, 128, 70 + 2 * step)
            m.train_step()
            out.append(_state(m) + [n.P.iterations.clone() for n in m.networks()])
        return m, out
    _, eager = run(False)
    mg, graph = run(True)
    assert mg._program is not None
    for step, (a, b) in enumerate(zip(eager, graph)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (step, i)


# ----------------------------------------------------------------------------- 5. CLI, checkpoints, pool, data parallel
def test_unet_cycle_cli_synthetic_directory_and_checkpoints(sg, tmp_path):
    from sggan_amd.main import main, parse_args, synthetic_batches
    base = ["--generator", "unet", "--cycle", "--paired", "1", "--batch_size", "1", "--img_height", "128", "--img_width", "128", "--ngf", "8", "--ndf", "8",
            "--dtype", "f32", "--steps_per_epoch", "2", "--log_dir", str(tmp_path / "logs")]
    # two epochs on synthetic batches through the CLI
    hist = main(base + ["--epoch", "2", "--dataset_dir", "unit", "--checkpoint_dir", str(tmp_path / "ck"), "--test_dir", str(tmp_path / "t")])
    assert len(hist) == 2 and all(np.isfinite([h["Generator Loss"], h["Discriminator Loss"]]).all() for h in hist)
    sd = torch.load(tmp_path / "ck" / "unit" / "gen" / "cp-0001.ckpt")
    assert sd["G"]["arch"] == "unet" and "G_BA" in sd and set(torch.load(tmp_path / "ck" / "unit" / "disc" / "cp-0001.ckpt")) == {"D", "D_B"}
    # resume: one epoch, save, reload into a new object, the second epoch == two uninterrupted epochs, for all four networks
    argv = base + ["--epoch", "2", "--dataset_dir", "unit", "--checkpoint_dir", str(tmp_path / "ck"), "--test_dir", str(tmp_path / "t")]
    ref = sg.sggan(parse_args(argv)); assert ref.load(str(tmp_path / "ck"))
    a1 = parse_args(argv); a1.epoch, a1.checkpoint_dir = 1, str(tmp_path / "ck2")
    m1 = sg.sggan(a1)
    m1.train(a1, synthetic_batches(m1, a1), log=lambda s: None)
    a2 = parse_args(argv); a2.epoch, a2.checkpoint_dir, a2.continue_train = 1, str(tmp_path / "ck2"), True
    m2 = sg.sggan(a2)
    second = synthetic_batches(m2, a2)
    m2.train(a2, lambda ep: second(1), log=lambda s: None)
    for x, y in zip(ref.networks(), m2.networks()):
        assert y.P.step_count == 4 and torch.equal(x.P.flat, y.P.flat) and torch.equal(x.P.m, y.P.m) and torch.equal(x.P.v, y.P.v)
    # a ResNet cycle checkpoint into the U-Net model, and the reverse, are refused by name
    r = parse_args([a for a in argv if a not in ("--generator", "unet")]); r.n_blocks = 2
    mr = sg.sggan(r)
    assert mr.arch == "resnet" and mr.cycle
    mr.save(str(tmp_path / "ckr"), 0)
    with pytest.raises(ValueError, match="resnet.*unet"):
        m2.load(str(tmp_path / "ckr"))
    with pytest.raises(ValueError, match="unet.*resnet"):
        mr.load(str(tmp_path / "ck"))
    # a dataset directory (domain B from the same root): two epochs in lockstep, then one with the U-Net's default sequencing (one
    # network at a time), the augmented copy, graph replay and the pool
    dirs = ["--generator", "unet", "--cycle", "--img_height", "128", "--img_width", "256", "--ngf", "8", "--ndf", "8", "--dataset_dir", FIX,
            "--dataset_dir_B", FIX, "--log_dir", str(tmp_path / "logs")]
    hist = main(dirs + ["--epoch", "2", "--paired", "1", "--checkpoint_dir", str(tmp_path / "ck3"), "--test_dir", str(tmp_path / "t3")])
    assert len(hist) == 2 and np.isfinite(hist[1]["Generator Loss"]) and np.isfinite(hist[1]["Discriminator Loss"])
    assert os.path.exists(tmp_path / "ck3" / "city_small" / "gen" / "cp-0001.ckpt") and os.path.exists(tmp_path / "t3" / "aachen_000016.png")
    hist = main(dirs + ["--epoch", "1", "--augment", "--graph", "--use_pool", "--checkpoint_dir", str(tmp_path / "ck4"),
                        "--test_dir", str(tmp_path / "t4")])
    assert len(hist) == 1 and np.isfinite(hist[0]["Generator Loss"]) and np.isfinite(hist[0]["Discriminator Loss"])


@pytest.mark.parametrize("mode", ["use_pool", "mixed", "checkpoint_blocks"])
def test_unet_cycle_step_mode_flags_run(sg, mode):
    """use_pool and mixed select the one-network-at-a-time sequencing (exactly as for the ResNet) and run with U-Nets;
    checkpoint_blocks is a no-op for the U-Net: the paired step, bit for bit the step without the flag."""
    kw = dict(use_resnet=False, ngf=8, ndf=8, dtype="bf16", cycle=True, paired=True)
    m = sg.sggan(sg.default_args(**kw, **{mode: True}))
    steps = 3 if mode == "use_pool" else 1
    for s in range(steps):
        _cycle_inputs(m, 1, 128, 128, 80 + 2 * s)
        m.train_step()
    assert all(np.isfinite(m.losses())) and all(torch.isfinite(n.P.flat).all() for n in m.networks())
    assert (getattr(m, "_pairs", None) is None) == (mode != "checkpoint_blocks")
    if mode == "checkpoint_blocks":
        assert not any(n.checkpoint_blocks for n in m.networks())
        p = sg.sggan(sg.default_args(**kw))
        _cycle_inputs(p, 1, 128, 128, 80)
        p.train_step()
        assert all(torch.equal(a, b) for a, b in zip(_state(m), _state(p)))


def test_unet_cycle_dp_world1_is_bit_identical_to_plain_step(sg):
    """tests/test_gpu_dp.py's world-size-1 pattern: the all-reduce launches hang on the U-Net's unit names (bucket_plan)."""
    import torch.distributed as dist
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        states = []
        for dp, graph in ((False, False), (True, False), (True, True)):
            m = sg.sggan(sg.default_args(use_resnet=False, ngf=16, ndf=16, dtype="f32", cycle=True, graph=graph, paired=True))
            if dp:
                m.enable_data_parallel()
            _cycle_inputs(m, 2, 128, 128, 90)
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                for _ in range(2):
                    m.train_step()
            assert not [w for w in caught if "Graph is empty" in str(w.message)], "an empty HIP-graph segment was recorded"
            plan = m.generator.bucket_plan(m.g_buckets)
            units = [f"e{i}" for i in range(1, 9)] + [f"d{i}" for i in range(1, 9)]
            assert len(plan) >= 3 and plan[0][:2] == ("e1", 0) and plan[-1][2] == m.generator.P.numel and all(p[0] in units for p in plan)
            if dp and graph:
                kinds = [k for k, _ in m._program.items]
                assert kinds.count("host") == 2 + len(plan) + 4   # two discriminator launches, one per generator bucket, four waits
            states.append(_state(m))
        for other in states[1:]:
            for x, y in zip(states[0], other):
                assert torch.equal(x, y)
    finally:
        dist.destroy_process_group()


# ----------------------------------------------------------------------------- 6. bf16 at full width
def test_unet_cycle_bf16_step_at_full_width_finite_and_close_to_f32(sg):
    """8x128x128, ngf 64: the bf16 step is finite and its losses are within 1e-2 (relative) of the f32 step on the same parameters
    and inputs -- test_unet_bf16_step_at_full_width_close_to_f32's bar."""
    out = {}
    for dtype in ("f32", "bf16"):
        m = sg.sggan(sg.default_args(use_resnet=False, ngf=64, ndf=64, dtype=dtype, cycle=True, paired=True))
        _cycle_inputs(m, 8, 128, 128, 7)
        m.train_step()
        out[dtype] = (m.losses(), torch.cat([n.P.grad for n in m.networks()]).double(), [n.P.flat.clone() for n in m.networks()])
        del m
        torch.cuda.empty_cache()
    (gl32, dl32), g32, _ = out["f32"]
    (gl16, dl16), g16, flats = out["bf16"]
    cos = float((g16 @ g32) / (g16.norm() * g32.norm()))
    print(f"bf16 vs f32 U-Net cycle step: g_loss {gl16:.5f}/{gl32:.5f} d_loss {dl16:.5f}/{dl32:.5f}, gradient cosine {cos:.5f}")
    assert all(np.isfinite([gl16, dl16])) and torch.isfinite(g16).all() and all(torch.isfinite(f).all() for f in flats)
    assert abs(gl16 - gl32) < 1e-2 * abs(gl32) and abs(dl16 - dl32) < 1e-2 * abs(dl32)


def test_unet_cycle_default_sequencing(sg):
    """paired=None (the default): lockstep for the ResNet; one network at a time for the U-Net, where lockstep is slower at
    256x512 batch 8 by more than the run-to-run spread; paired=True / --paired 1 selects the pair path."""
    from sggan_amd.main import parse_args
    kw = dict(ngf=8, ndf=8, n_blocks=1, cycle=True)
    assert sg.sggan(sg.default_args(**kw)).paired is True
    assert sg.sggan(sg.default_args(use_resnet=False, **kw)).paired is False
    assert sg.sggan(sg.default_args(use_resnet=False, paired=True, **kw)).paired is True
    a = parse_args(["--generator", "unet", "--cycle", "--ngf", "8", "--ndf", "8"])
    assert a.paired is None and sg.sggan(a).paired is False
    a = parse_args(["--generator", "unet", "--cycle", "--ngf", "8", "--ndf", "8", "--paired", "1"])
    assert sg.sggan(a).paired is True
