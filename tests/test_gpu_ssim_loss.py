"""GPU tests of the structural-similarity training loss (--ssim_lambda): the kernels of csrc/ssimloss.hip against
the float64 statement (tests/ssim_loss_oracle.py) at their tile edges, their exactness and memory discipline, the autograd op, the
reference and the cycle step with the term against float64 restatements, and the paths the option must survive (graph replay,
paired / one-at-a-time cycle, U-Net, the command line)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import sggan_oracle as O
from tests import ssim_loss_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
SL_TH, SL_TW = 16, 32           # windows of a forward block = pixels of an adjoint block (csrc/ssimloss.hip; test_ssim_loss_cpu.py checks)
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
# one window (every pixel fed by exactly one); one more window on either axis; the first size where a pixel collects all 11 windows
# on each axis and has a neighbour that does too; exactly one full window tile; 2 x 2 window tiles with one-window tails; 3 x 3
# window tiles, two full plus a tail on each axis (and 3 x 3 pixel tiles of the adjoint launch)
SHAPES = [(11, 11), (11, 12), (12, 11), (21, 22), (26, 42), (27, 43), (43, 75)]
GUARD = 256                     # bytes in front of and behind dx and ws that must keep their pattern
WEIGHT, GSCALE = 5.0, 0.5


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


def _grid(rng, shape):
    """Values in [0, 1] on the 1/64 grid: exact in bf16 (8 significant bits) and f32."""
    return rng.integers(0, 65, shape).astype(np.float64) / 64.0


def _to_dev(a, dtype, pad_value=0.0):
    """(N,H,W,C) float64 -> the internal layout (8 channels); the padded channels carry ``pad_value``."""
    t = torch.full(a.shape[:3] + (8,), pad_value, dtype=torch.float64)
    t[..., :a.shape[3]] = torch.from_numpy(a)
    return t.to(TORCH_DT[dtype]).to(DEV).contiguous()


def _ulp(v, dtype):
    """The spacing of the storage type at |v| (24 / 8 significant bits; below the smallest normal, the subnormal spacing)."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 2.0 ** (e - (23 if dtype == "f32" else 7))


class _Guarded:
    """A device buffer of ``nbytes`` with GUARD bytes of a pattern on either side; ``view(dtype, shape)`` is the inside."""

    def __init__(self, nbytes, fill=0xFF):
        self.nbytes = nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.raw[GUARD:GUARD + nbytes] = fill                               # 0xFF: NaN in f32, bf16 and double
        assert self.raw.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr() + GUARD)

    def inside(self):
        return self.raw[GUARD:GUARD + self.nbytes]

    def view(self, dtype, shape):
        return self.inside().view(dtype).view(shape)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xA5).all())


def _raw_call(t, x, Cr, loss, dx_ptr, acc, ws, nbytes=None, weight=WEIGHT, gscale=GSCALE, data_range=1.0):
    from sggan_amd import _abi as A
    from sggan_amd import kernels as K
    N, H, W, Cp = x.shape
    return A.lib().sgg_ssim_loss(K._p(t), K._p(x), N, H, W, Cr, Cp, data_range, weight, gscale, K._p(loss), dx_ptr, acc, K.dt(x),
                                 ws.ptr, ws.nbytes if nbytes is None else nbytes, K._s())


def _check_dx(name, got, exact, M, dtype):
    """The kernel keeps everything in double up to ONE rounding to the storage type, so a stored value lies within half a storage
    ulp of the exact  dx_old + g  (g = gscale * weight * dL/dx), plus
      * 2^-53 |dx_old + g| for the one double addition that joins dx_old and g when accumulating (also the slack for a double that
        sits within its own rounding of a storage tie), and
      * 64 * 2^-53 * M[q] * |gscale * weight| for the order of the sums: the kernel's fma chains and this file's NumPy sums add the
        same ~ 3 * 121 products of total size M in different orders, each within a few double roundings of the true sum.
    Nothing here was tuned on a GPU result."""
    err = np.abs(got - exact)
    bound = 0.5 * _ulp(exact, dtype) + 2.0 ** -53 * np.abs(exact) + 64 * 2.0 ** -53 * M * abs(GSCALE * WEIGHT)
    worst = float((err / bound).max())
    print(f"{name} [{dtype}]: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.all(err <= bound), (name, worst, int((err > bound).sum()))


def _check_loss(name, got, exact):
    """One rounding to f32 of a double that carries the order-of-sums error of the mean (far below an f32 ulp): 1 ulp of f32."""
    ulp = float(_ulp(np.float64(exact), "f32"))
    print(f"{name}: loss {got!r} vs {exact!r}, |err| / ulp {abs(got - exact) / ulp:.3f}")
    assert abs(got - exact) <= ulp, (name, got, exact)


def _bits(t):
    return t.contiguous().view(torch.uint8).clone()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_against_the_float64_statement(sg, hw, N, dtype):
    _kernel_case(hw, N, 3, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("Cr", [1, 8])
def test_kernel_with_one_and_with_all_eight_real_channels(sg, Cr, dtype):
    _kernel_case((27, 43), 2, Cr, dtype)


def _kernel_case(hw, N, Cr, dtype):
    from sggan_amd import _abi as A
    H, W = hw
    assert (SL_TH + 10, SL_TW + 10) == (26, 42)
    rng = np.random.default_rng(1000 * H + 10 * W + N + 7 * Cr)
    t, x = _grid(rng, (N, H, W, Cr)), _grid(rng, (N, H, W, Cr))
    old = _grid(rng, (N, H, W, Cr)) * 2.0 ** -10 - 2.0 ** -11                  # dx_old: exact in bf16, of the gradient's size
    td, xd = _to_dev(t, dtype, 7.0), _to_dev(x, dtype, float("nan"))           # (garbage in the padded channels)
    keep_t, keep_x = _bits(td), _bits(xd)
    esize = 4 if dtype == "f32" else 2
    L = SO.loss(t, x)
    g = GSCALE * WEIGHT * SO.grad(t, x)
    M = SO.magnitude(t, x)
    need = int(A.lib().sgg_ssim_loss_workspace(N, H, W, Cr))
    assert need == 8 * (N * Cr * 3 * (H - 10) * (W - 10) + N * (-(-(H - 10) // SL_TH)) * (-(-(W - 10) // SL_TW)))

    results = {}
    for acc in (0, 1, 2, 3):
        ws = _Guarded(need)
        dxb = _Guarded(N * H * W * 8 * esize)
        dx = dxb.view(TORCH_DT[dtype], (N, H, W, 8))
        if acc & 2:
            dx[..., :Cr] = torch.from_numpy(old).to(TORCH_DT[dtype]).to(DEV)   # (padded channels stay NaN)
        before = _bits(dx)
        loss = torch.tensor([0.75 if acc & 1 else float("nan")], dtype=torch.float32, device=DEV)
        assert _raw_call(td, xd, Cr, loss, dxb.ptr, acc, ws) == A.OK
        torch.cuda.synchronize()
        assert ws.guards_intact() and dxb.guards_intact()
        assert torch.equal(_bits(td), keep_t) and torch.equal(_bits(xd), keep_x)
        _check_loss(f"acc={acc}", float(loss.item()), (0.75 if acc & 1 else 0.0) + WEIGHT * L)
        got = dx[..., :Cr].to(torch.float64).cpu().numpy()
        _check_dx(f"dx acc={acc}", got, (old if acc & 2 else 0.0) + g, M, dtype)
        if acc & 2:
            assert torch.equal(_bits(dx).view(N, H, W, 8, esize)[..., Cr:, :], before.view(N, H, W, 8, esize)[..., Cr:, :])   # padded channels: not touched
        elif Cr < 8:
            assert bool((dx[..., Cr:] == 0).all()) and not bool(torch.signbit(dx[..., Cr:]).any())             # written as +0
        results[acc] = (_bits(loss), _bits(dx))
        # a second run on fresh NaN-filled buffers gives the same bits
        ws2, dxb2 = _Guarded(need), _Guarded(N * H * W * 8 * esize)
        dx2 = dxb2.view(TORCH_DT[dtype], (N, H, W, 8))
        dx2.view(torch.uint8).copy_(before)
        loss2 = torch.tensor([0.75 if acc & 1 else float("nan")], dtype=torch.float32, device=DEV)
        assert _raw_call(td, xd, Cr, loss2, dxb2.ptr, acc, ws2) == A.OK
        assert torch.equal(_bits(loss2), results[acc][0]) and torch.equal(_bits(dx2), results[acc][1])

    # dx == NULL: the loss alone, the same bits, and nothing of the coefficient maps is written
    ws = _Guarded(need)
    loss = torch.tensor([float("nan")], dtype=torch.float32, device=DEV)
    assert _raw_call(td, xd, Cr, loss, None, 0, ws) == A.OK
    assert torch.equal(_bits(loss), results[0][0]) and ws.guards_intact()
    coef_bytes = 8 * N * Cr * 3 * (H - 10) * (W - 10)
    assert bool((ws.inside()[:coef_bytes] == 0xFF).all())

    # refused calls leave loss and dx alone
    dxb = _Guarded(N * H * W * 8 * esize)
    loss = torch.tensor([float("nan")], dtype=torch.float32, device=DEV)
    assert _raw_call(td, xd, Cr, loss, dxb.ptr, 0, ws, nbytes=need - 1) == A.EWORKSPACE
    assert _raw_call(td, xd, Cr, loss, dxb.ptr, 0, ws, data_range=0.0) == A.EINVAL
    assert _raw_call(td, xd, Cr, loss, ctypes.c_void_p(xd.data_ptr()), 0, ws) == A.EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and bool((dxb.inside() == 0xFF).all()) and torch.equal(_bits(xd), keep_x)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_identical_operands_give_a_loss_of_exactly_zero(sg, dtype):
    """S == 1.0 exactly in every window (numerator and denominator are the same expressions of the same values), also on a
    piecewise-constant image, where E[xx] - ux^2 cancels to rounding noise; the gradient's coefficients vanish with it."""
    from sggan_amd import kernels as K
    rng = np.random.default_rng(11)
    x = _grid(rng, (2, 43, 75, 3))
    x[0, :, :40] = 0.25
    x[1, 10:30] = 0.0
    xd = _to_dev(x, dtype)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    dx = torch.full_like(xd, float("nan"))
    K.ssim_loss(xd.clone(), xd, 3, loss, dx, weight=WEIGHT)
    assert _bits(loss).tolist() == [0, 0, 0, 0]                                # +0.0f
    assert bool(torch.isfinite(dx).all()) and float(dx.abs().max()) <= 1e-12   # (alpha + x * (beta + gamma) cancels to rounding)
    loss.fill_(float("nan"))
    K.ssim_loss(xd.clone(), xd, 3, loss, None, weight=WEIGHT, data_range=255.0)
    assert _bits(loss).tolist() == [0, 0, 0, 0]


def test_autograd_op_value_and_gradient_are_the_kernels(sg):
    from sggan_amd import kernels as K
    rng = np.random.default_rng(3)
    t, x = _grid(rng, (2, 27, 43, 3)), _grid(rng, (2, 27, 43, 3))
    xt = torch.from_numpy(x).float().to(DEV).requires_grad_(True)
    tt = torch.from_numpy(t).float().to(DEV)
    y = sg.ssim_loss(xt, tt)
    assert y.dim() == 0
    (3.0 * y).backward()
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    dx = torch.empty((2, 27, 43, 8), dtype=torch.float32, device=DEV)
    K.ssim_loss(_to_dev(t, "f32"), _to_dev(x, "f32"), 3, loss, dx)
    assert torch.equal(y.detach().reshape(1), loss) and torch.equal(xt.grad, dx[..., :3] * 3.0)
    _check_loss("op", y.item(), SO.loss(t, x))
    with torch.no_grad():                                                     # no gradient asked: the loss-only form
        assert torch.equal(sg.ssim_loss(xt.detach(), tt).reshape(1), loss)
    y2 = sg.ssim_loss(xt, tt, data_range=2.0)
    _check_loss("op, data_range 2", y2.item(), SO.loss(t, x, 2.0))
    with pytest.raises(ValueError):
        sg.ssim_loss(xt, tt[:, :, :, :2])


# ---- the steps with the term ------------------------------------------------------------------------------------------------
def _rand_inputs(N, H, W, D, seed):
    g = torch.Generator().manual_seed(seed)
    real = torch.rand((N, H, W, 3), generator=g)
    seg = torch.rand((N, H, W, 3), generator=g)
    mh, mw = D.out_hw(H, W)
    mh, mw = (4, 4) if (mh, mw) == (1, 1) else (mh, mw)
    idx = torch.randint(0, 34, (N, mh, mw), generator=g)
    return real, seg, torch.nn.functional.one_hot(idx, 34).float()


def _feed(m, step=0, N=2, H=128, W=128):
    m.real_A, m.seg_A, m.mask_A = _rand_inputs(N, H, W, m.discriminator, 40 + step)
    if m.cycle:
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(N, H, W, m.discriminator, 50 + step)


def _state(m):
    return [t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.iterations, n.P.grad)] + [m._loss.clone()]


def _rel(got, exp):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    return np.abs(got - exp).max() / max(np.abs(exp).max(), 1e-12)


def _l2(a, b):
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-300))


def test_reference_step_with_the_term_against_the_float64_restatement(sg):
    """One reference step (f32, reduced widths, 128x128: the smallest size the discriminator accepts, ssim_lambda 5) against
    oracle.train_step with the term as one more taped op, evaluated kink-aware (tests/kink_helpers.py).  Bounds of
    tests/test_gpu_step.py::test_train_step_small_f32_matches_oracle: 1e-5 on the losses, 1e-4 on the images, 2e-4 on every
    gradient tensor (relative L2 and worst entry / largest entry)."""
    from tests.kink_helpers import discriminator_branches, generator_branches
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="f32", keep_tapes=True, ssim_lambda=5.0))
    assert m.ssim_lambda == 5.0 and m.ssim_data_range == 1.0
    G_, D_ = m.generator, m.discriminator
    PG = {k: v.astype(np.float64) for k, v in G_.P.export().items()}
    PD = {k: v.astype(np.float64) for k, v in D_.P.export().items()}
    real, seg, mask = _rand_inputs(2, 128, 128, D_, 7)
    m.real_A, m.seg_A, m.mask_A = real, seg, mask
    m.train_step()
    gl, dl = m.losses()
    t = m.tapes
    branches = generator_branches(G_, t["G"]) + discriminator_branches(D_, t["D_real"]) + discriminator_branches(D_, t["D_fake"])
    f64 = lambda a: a.numpy().astype(np.float64)
    pol = O.KinkPolicy(1e-4, branches)
    O.KINKS = pol
    try:
        r = SO.train_step(PG, PD, f64(real), f64(seg), f64(mask), 5.0, n_blocks=1)
    finally:
        O.KINKS = None
    assert pol.calls == len(branches) and pol.disagree_outside == 0
    pol = O.KinkPolicy(1e-4, branches)
    O.KINKS = pol
    try:
        r0 = SO.train_step(PG, PD, f64(real), f64(seg), f64(mask), 0.0, n_blocks=1)
    finally:
        O.KINKS = None
    print(f"gen_loss {gl!r} vs {r['gen_loss']!r} (without the term {r0['gen_loss']!r}); disc_loss {dl!r} vs {r['disc_loss']!r}")
    assert abs(gl - r["gen_loss"]) < 1e-5 * abs(r["gen_loss"]) and abs(dl - r["disc_loss"]) < 1e-5 * abs(r["disc_loss"])
    assert _rel(m.fake_A.numpy(), r["fake_A"]) < 1e-4
    assert _rel(m.da_real.detach().cpu().numpy(), r["da_real"]) < 1e-4 and _rel(m.da_fake.detach().cpu().numpy(), r["da_fake"]) < 1e-4
    # sensitivity: the term moves the generator's loss and its last layer's gradient by more than the bounds
    assert abs(r["gen_loss"] - r0["gen_loss"]) > 1e-3 * abs(r0["gen_loss"])
    last = [k for k in r["gG"] if k.startswith("out_")]
    assert last and all(_rel(r["gG"][k], r0["gG"][k]) > 2e-4 for k in last), [(k, _rel(r["gG"][k], r0["gG"][k])) for k in last]
    worst = {}
    for label, got_all, exp_all, keep in (("gD", D_.P.export(D_.P.grad), r["gD"], ("h0_b", "h4_b")), ("gG", G_.P.export(G_.P.grad), r["gG"], ("out_b",))):
        for k, v in got_all.items():
            e = exp_all[k]
            if k.endswith("_b") and k not in keep:           # bias in front of an InstanceNorm: exactly 0 here, ~1e-16 in float64
                assert np.abs(v).max() == 0.0 and np.abs(e).max() < 1e-9
                continue
            worst[(label, k)] = (_l2(v.astype(np.float64), e), _rel(v, e))
    print("worst tensors (relative L2, worst entry / largest entry):",
          [(k, "%.1e" % a, "%.1e" % b) for k, (a, b) in sorted(worst.items(), key=lambda kv: -kv[1][0])[:5]])
    assert all(a < 2e-4 and b < 2e-4 for a, b in worst.values()), {k: v for k, v in worst.items() if max(v) >= 2e-4}


@pytest.mark.parametrize("d_quad", [False, True], ids=["two_passes", "d_quad"])
@pytest.mark.parametrize("use_lsgan", [True, False], ids=["lsgan", "sce"])
def test_cycle_step_with_the_term_against_the_float64_restatement(sg, use_lsgan, d_quad):
    """One paired cycle step (f32, LSGAN and SCE, reduced networks, 128x128, ssim_lambda 5) against the cycle restatement with the
    two extra terms, kink-aware, for both sequencings of the discriminators -- the cases and bounds of
    tests/test_gpu_step.py::test_cycle_step_small_f32_matches_oracle: 2e-5 on the losses, 1e-4 / 2e-4 on fakes / reconstructions,
    2e-4 on every gradient tensor (relative L2 and worst entry / largest entry)."""
    from tests.kink_helpers import cycle_step_branches
    N, H, W, ngf, ndf, n_blocks = 1, 128, 128, 8, 8, 1
    rng = np.random.default_rng(29)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    gs = O.generator_param_shapes(gf_dim=ngf, n_blocks=n_blocks); ds = O.discriminator_param_shapes(df_dim=ndf)
    P = {n: {k: f32(v) for k, v in O.init_params(sh, rng, 0.1).items()} for n, sh in (("Gab", gs), ("Gba", gs), ("Da", ds), ("Db", ds))}
    real_A, real_B = f32(rng.uniform(0, 1, (N, H, W, 3))), f32(rng.uniform(0, 1, (N, H, W, 3)))
    pal = rng.integers(0, 256, (8, 3)) / 255.0
    blocks = lambda: f32(pal[np.repeat(np.repeat(rng.integers(0, 8, (N, H // 32, W // 32)), 32, 1), 32, 2)])
    seg_A, seg_B = blocks(), blocks()
    mk = lambda: np.stack([O.one_hot(i, 34) for i in rng.integers(0, 34, (N, 4, 4))]).astype(np.float64)
    mask_A, mask_B = mk(), mk()
    m = sg.sggan(sg.default_args(ngf=ngf, ndf=ndf, n_blocks=n_blocks, dtype="f32", cycle=True, use_lsgan=use_lsgan, keep_tapes=True, d_quad=d_quad,
                                 ssim_lambda=5.0))
    assert m.d_quad == d_quad and m.paired
    nets = {"Gab": m.generator, "Gba": m.generator_BA, "Da": m.discriminator, "Db": m.discriminator_B}
    for n, net in nets.items():
        net.P.load(P[n])
    m.real_A, m.real_B, m.seg_A, m.seg_B, m.mask_A, m.mask_B = real_A, real_B, seg_A, seg_B, mask_A, mask_B
    m.train_step()
    gl, dl = m.losses()
    assert (m.tapes["D_quad"] is not None) == d_quad
    branches = cycle_step_branches(m)
    out = []
    for lam in (5.0, 0.0):
        pol = O.KinkPolicy(1e-4, branches)
        O.KINKS = pol
        try:
            out.append(SO.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], real_A, real_B, seg_A, seg_B, mask_A, mask_B, lam, use_lsgan=use_lsgan,
                                     n_blocks=n_blocks))
        finally:
            O.KINKS = None
        assert pol.calls == len(branches) and pol.disagree_outside == 0
    r, r0 = out
    print(f"g_loss {gl!r} vs {r['g_loss']!r} (without the term {r0['g_loss']!r}); d_loss {dl!r} vs {r['d_loss']!r}")
    assert abs(gl - r["g_loss"]) < 2e-5 * abs(r["g_loss"]) and abs(dl - r["d_loss"]) < 2e-5 * abs(r["d_loss"])
    assert _rel(m.fake_B.numpy(), r["fake_B"]) < 1e-4 and _rel(m.cyc_A.numpy(), r["cyc_A"]) < 2e-4
    assert _rel(m.fake_A.numpy(), r["fake_A"]) < 1e-4 and _rel(m.cyc_B.numpy(), r["cyc_B"]) < 2e-4
    assert abs(r["g_loss"] - r0["g_loss"]) > 1e-3 * abs(r0["g_loss"])
    for n in ("Gab", "Gba"):                                  # sensitivity: the last layer's gradient moves by more than the bound
        last = [k for k in r["grads"][n] if k.startswith("out_")]
        assert last and all(_rel(r["grads"][n][k], r0["grads"][n][k]) > 2e-4 for k in last)
    worst = {}
    for n, net in nets.items():
        got = net.P.export(net.P.grad)
        for k, e in r["grads"][n].items():
            if np.abs(e).max() < 1e-9:
                continue
            worst[(n, k)] = (_l2(got[k].astype(np.float64), e), _rel(got[k], e))
    print("largest gradient errors (relative L2, worst entry):",
          [(k, "%.1e" % v[0], "%.1e" % v[1]) for k, v in sorted(worst.items(), key=lambda kv: -kv[1][0])[:4]])
    bad = {k: v for k, v in worst.items() if not (v[0] < 2e-4 and v[1] < 2e-4)}
    assert not bad, bad


# ---- the paths the option must survive ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "paired_cycle"])
def test_graph_replay_equals_eager_bitwise_with_the_option(sg, cycle):
    """3 steps, bf16: the term's three launches per call are part of the recorded step."""
    def run(graph):
        m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=cycle, graph=graph, ssim_lambda=2.0))
        out = []
        for step in range(3):
            _feed(m, step)
            m.train_step()
            out.append(_state(m) + [m.fake_A.tensor().clone()])
        return m, out
    me, eager = run(False)
    mg, graph = run(True)
    assert mg._program is not None and mg._program.n_graphs >= 1 and (not cycle or mg.paired)
    for step, (a, b) in enumerate(zip(eager, graph)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (step, i)
    plain = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=cycle))
    _feed(plain, 0)
    plain.train_step()
    assert not torch.equal(plain._loss[0:1], eager[0][-2][0:1])                # the option is really on


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paired_cycle_step_equals_one_network_at_a_time_with_the_option(sg, dtype):
    """The bounds of test_paired_cycle_step_is_bit_identical_to_one_network_at_a_time (d_quad off): losses and images bitwise;
    parameter / slot / gradient buffers equal or within 1e-5 of their norm (shared weight-gradient launches)."""
    out, names = [], None
    for paired in (False, True):
        m = sg.sggan(sg.default_args(ngf=16, ndf=16, n_blocks=2, dtype=dtype, cycle=True, paired=paired, d_quad=False, ssim_lambda=5.0))
        m.real_A, m.seg_A, m.mask_A = _rand_inputs(2, 128, 128, m.discriminator, 61)
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(2, 128, 128, m.discriminator, 62)
        m.train_step()
        names = [f"net{k}.{what}" for k, n in enumerate(m.networks()) for what in ("flat", "m", "v", "grad")] + ["loss", "fake_A", "fake_B", "cyc_A", "cyc_B"]
        out.append([t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.grad)] +
                   [m._loss.clone(), m.fake_A.tensor(), m.fake_B.tensor(), m.cyc_A.tensor(), m.cyc_B.tensor()])
    for name, a, b in zip(names, *out):
        if torch.equal(a, b):
            continue
        assert name.startswith("net"), name
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        assert rel < 1e-5, (name, rel)


def test_data_parallel_halves_average_to_the_full_batch_with_the_option(sg):
    """The term is a mean over (image, channel, window), so -- like L1 -- the mean of two half-batch generator gradients is the
    full-batch one; the bound is tests/test_gpu_step.py::test_step_is_deterministic_and_dp_equivalent's for the generator."""
    args = sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="f32", ssim_lambda=5.0)
    full = sg.sggan(args)
    real, seg, mask = _rand_inputs(4, 128, 128, full.discriminator, 7)
    full.real_A, full.seg_A, full.mask_A = real, seg, mask
    full.train_step()
    acc, loss = torch.zeros_like(full.generator.P.grad), 0.0
    for sl in (slice(0, 2), slice(2, 4)):
        h = sg.sggan(args)
        h.real_A, h.seg_A, h.mask_A = real[sl], seg[sl], mask[sl]
        h.train_step()
        acc += h.generator.P.grad / 2
        loss += h.losses()[0] / 2
    assert (acc - full.generator.P.grad).abs().max() < 1e-4 * full.generator.P.grad.abs().max()
    assert abs(loss - full.losses()[0]) < 1e-5 * abs(full.losses()[0])


def test_unet_cycle_step_and_pool_step_run_with_the_option(sg):
    for kw in (dict(use_resnet=False), dict(use_pool=True, n_blocks=1)):
        m = sg.sggan(sg.default_args(ngf=8, ndf=8, dtype="bf16", cycle=True, ssim_lambda=2.0, **kw))
        _feed(m)
        m.train_step()
        gl, dl = m.losses()
        assert np.isfinite(gl) and np.isfinite(dl), kw
        assert all(bool(torch.isfinite(n.P.flat).all()) for n in m.networks()), kw


def test_command_line_runs_one_synthetic_epoch_with_the_option(sg, tmp_path):
    from sggan_amd.main import main
    hist = main(["--cycle", "--ssim_lambda", "2", "--batch_size", "1", "--img_height", "128", "--img_width", "128", "--ngf", "8", "--ndf", "8",
                 "--steps_per_epoch", "2", "--epoch", "1", "--dataset_dir", "unit", "--log_dir", str(tmp_path / "logs"),
                 "--checkpoint_dir", str(tmp_path / "ck"), "--test_dir", str(tmp_path / "t")])
    assert len(hist) == 1 and np.isfinite([hist[0]["Generator Loss"], hist[0]["Discriminator Loss"]]).all()


def test_bad_values_and_undersized_images_are_refused_with_a_value_error(sg):
    kw = dict(ngf=8, ndf=8, n_blocks=1)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ssim_lambda"):
            sg.sggan(sg.default_args(ssim_lambda=bad, **kw))
    with pytest.raises(ValueError, match="ssim_data_range"):
        sg.sggan(sg.default_args(ssim_lambda=1.0, ssim_data_range=0.0, **kw))
    with pytest.raises(ValueError, match="--ssim_lambda"):
        sg.sggan(sg.default_args(ssim_lambda=1.0, image_height=8, image_width=128, **kw))
    m = sg.sggan(sg.default_args(ssim_lambda=1.0, **kw))
    m.real_A, m.seg_A, m.mask_A = torch.rand(1, 10, 128, 3), torch.rand(1, 10, 128, 3), torch.zeros(1, 4, 4, 34)
    with pytest.raises(ValueError, match="--ssim_lambda"):
        m.train_step()
    off = sg.sggan(sg.default_args(**kw))                                       # off: nothing of the option exists
    assert off.ssim_lambda == 0.0
