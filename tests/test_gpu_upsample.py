"""GPU tests of the resize-convolution option of generator_resnet: the 2x resampling kernels bit for bit, under
graph capture and through autograd; the two new units, the generator and both train steps against the float64 statement of
tests/upsample_oracle.py; the bitwise identities the option must keep; checkpoint tags; launch counts; the weight average."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sggan_oracle as O
from tests import unit_spy
from tests import upsample_oracle as UO

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


# ----------------------------------------------------------------------------- 1. the kernels, bit for bit
# csrc/upsample.hip: UP_THREADS = 256, UP_CHUNK = 256 low-resolution vectors of 8 channels per block and grid stride (one per thread),
# UP_GRID_BLOCKS = 1024 -- the grid cap is reached at 1024 * 256 = 262144 vectors (tests/test_upsample_cpu.py holds kernels.py's copies
# of the three to the source).  Shapes are (N,H,W,Cp) of the LOW-resolution tensor, N*H*W*Cp/8 vectors (2.1 M elements at the cap):
SHAPES = [(1, 1, 1, 8), (1, 1, 2, 8), (1, 2, 1, 8), (2, 3, 5, 24), (1, 4, 7, 64),
          (1, 3, 85, 8), (1, 2, 16, 64), (1, 1, 257, 8),                    # 255, 256, 257 vectors: below, at, above one chunk
          (1, 189, 1387, 8), (1, 64, 128, 256), (1, 65, 4033, 8)]           # 262143, 262144, 262145: below, at, above the grid cap
GUARD = 64                                                                   # elements around every output


def _vectors(shape):
    return int(np.prod(shape)) // 8


def test_shapes_sit_on_the_kernels_edges(sg):
    K = sg.kernels
    assert (K.UPSAMPLE_CHUNK, K.UPSAMPLE_GRID_BLOCKS) == (256, 1024)
    assert [_vectors(s) for s in SHAPES[5:]] == [255, 256, 257, 262143, 262144, 262145]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device="cuda", dtype=dtype)


def _guarded(shape, dtype):
    """(flat buffer pre-filled with a sentinel, its middle viewed as ``shape``): GUARD cells on either side."""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), -77.0, dtype=dtype, device="cuda")
    return flat, flat[GUARD:GUARD + n].view(shape)


def _run(K, direction, a, mode, dtype):
    """The kernel on the f32 array a (values of the storage type) -> (float32 array, the guard cells were left alone)."""
    x = _dev(a, dtype)
    N, H, W, Cp = x.shape
    shape = (N, 2 * H, 2 * W, Cp) if direction == "fwd" else (N, H // 2, W // 2, Cp)
    flat, out = _guarded(shape, dtype)
    (K.upsample2x if direction == "fwd" else K.upsample2x_bwd)(x, mode, out=out)
    torch.cuda.synchronize()
    guards_ok = bool((flat[:GUARD] == -77.0).all() and (flat[-GUARD:] == -77.0).all())
    return out.to(torch.float32).cpu().numpy(), guards_ok


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("mode", UO.MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_kernels_bitwise(sg, dtype, mode, shape):
    """Forward and adjoint: exact on integer inputs (x in [-15,15], dy in [-3,3]: every value is exact in bf16); on random inputs
    the nearest forward is the index gather, everything else equals the f32 emulation of the kernel's tap order bit for bit and
    lies inside the derived bound of the float64 operator; the guard cells around every output keep their sentinel."""
    K, bf16 = sg.kernels, dtype == "bf16"
    N, H, W, Cp = shape
    rng = np.random.default_rng(_vectors(shape) + len(mode))
    store = (lambda a: UO._bf16(a)) if bf16 else (lambda a: a.astype(np.float32))
    xi, gi = rng.integers(-15, 16, shape).astype(np.float32), rng.integers(-3, 4, (N, 2 * H, 2 * W, Cp)).astype(np.float32)
    xr, gr = store(rng.standard_normal(shape)), store(rng.standard_normal((N, 2 * H, 2 * W, Cp)))
    for direction, ints, rand, emu, op in (("fwd", xi, xr, UO.emulate_fwd, UO.up), ("bwd", gi, gr, UO.emulate_bwd, UO.up_T)):
        got, ok = _run(K, direction, ints, mode, DT[dtype])
        assert ok and np.array_equal(got, op(ints, mode)), (direction, "integers")
        got, ok = _run(K, direction, rand, mode, DT[dtype])
        assert ok, (direction, "guards")
        if (mode, direction) == ("nearest", "fwd"):
            gather = rand[:, np.arange(2 * H) >> 1][:, :, np.arange(2 * W) >> 1]
            assert np.array_equal(got.view(np.uint32), gather.view(np.uint32))
            continue
        exact, bnd = UO.bound(rand, mode, direction, bf16)
        ratio = float((np.abs(got - exact) / bnd).max())
        same = np.array_equal(got.view(np.uint32), emu(rand, mode, bf16).view(np.uint32))
        print(f"{dtype} {mode} {direction} {shape}: worst |err| / bound {ratio:.3f}, equals the f32 emulation: {same}")
        assert ratio <= 1.0 and same, (direction, ratio, same)


# ----------------------------------------------------------------------------- 2. graph capture
@pytest.mark.parametrize("mode", UO.MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_kernels_replay_to_eagers_bits(sg, dtype, mode):
    K = sg.kernels
    g_ = torch.Generator().manual_seed(7)
    x = torch.randn((2, 9, 33, 24), generator=g_).to(device="cuda", dtype=DT[dtype])
    dy = torch.randn((2, 18, 66, 24), generator=g_).to(device="cuda", dtype=DT[dtype])
    y0, dx0 = K.upsample2x(x, mode), K.upsample2x_bwd(dy, mode)
    y1, dx1 = torch.zeros_like(y0), torch.zeros_like(dx0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.upsample2x(x, mode, out=y1)
        K.upsample2x_bwd(dy, mode, out=dx1)
    for _ in range(2):
        y1.zero_(); dx1.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y0, y1) and torch.equal(dx0, dx1)


# ----------------------------------------------------------------------------- 3. the autograd op
@pytest.mark.parametrize("mode", UO.MODES)
def test_ops_upsample2x_against_interpolate(sg, mode):
    """ops.upsample2x (f32, 3 real channels: padded on the way in, cropped on the way out) against torch's interpolate and ITS
    autograd gradient in float64, inside the derived bound."""
    g_ = torch.Generator().manual_seed(11)
    x = torch.randn((2, 5, 7, 3), generator=g_)
    gy = torch.randn((2, 10, 14, 3), generator=g_)
    xd = x.cuda().requires_grad_(True)
    y = sg.ops.upsample2x(xd, mode)
    y.backward(gy.cuda())
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    yr = F.interpolate(xr, scale_factor=2, mode=mode, **({} if mode == "nearest" else {"align_corners": False}))
    yr.backward(gy.double().permute(0, 3, 1, 2))
    assert tuple(y.shape) == (2, 10, 14, 3) and y.dtype == torch.float32
    if mode == "nearest":
        assert np.array_equal(y.detach().cpu().numpy(), yr.detach().permute(0, 2, 3, 1).numpy().astype(np.float32))
    else:
        exact, bnd = UO.bound(x.numpy(), mode, "fwd", False)
        assert np.abs(exact - yr.detach().permute(0, 2, 3, 1).numpy()).max() < 1e-14
        assert (np.abs(y.detach().cpu().numpy() - exact) <= bnd).all()
    exact, bnd = UO.bound(gy.numpy(), mode, "bwd", False)
    assert np.abs(exact - xr.grad.permute(0, 2, 3, 1).numpy()).max() < 1e-13
    assert (np.abs(xd.grad.cpu().numpy() - exact) <= bnd).all()
    with pytest.raises(ValueError, match="mode"):
        sg.ops.upsample2x(xd, "cubic")


# ----------------------------------------------------------------------------- 4. the two new units alone
UNIT_CASES = [(name, w, dtype) for name in ("d1", "d2") for w in (64, 32) for dtype in ("bf16", "f32")]


def _unit_inputs(name, w_in, dtype, n, seed):
    cin = 256 if name == "d1" else 128
    g_ = torch.Generator().manual_seed(seed)
    h = torch.randn((n, 2, w_in, cin), generator=g_).to(device="cuda", dtype=DT[dtype])
    dy = (0.1 * torch.randn((n, 4, 2 * w_in, cin // 2), generator=g_)).to(device="cuda", dtype=DT[dtype])
    return h, dy


def _check_unit(sg, unit, h, dy, dtype, mode, route):
    """Resample, run the unit forward and backward under the recorder, hold every stage to tests/unit_oracle.py's bounds."""
    K, A = sg.kernels, sg._abi
    g = unit.geom(K.upsample2x(h, mode))
    fwd = A.route_name(g.route_fwd)
    assert (fwd == "HALO3") if route == "HALO3" else fwd.startswith("GLDS_"), fwd
    nets = [unit.ua.net, unit.ub.net] if hasattr(unit, "ua") else [unit.net]
    for net in nets:
        net.P.zero_grad()
    with unit_spy.Spy(SimpleNamespace(conv_units=lambda: [unit]), A.route_name) as spy:
        y, rec = unit.forward(K.upsample2x(h, mode))
        unit.backward(rec, dy, True, True)
    report = {}
    results = unit_spy.check(spy, dtype, report)
    print(f"{unit.name} {dtype} {mode} route {fwd}: worst ratio per stage", {k: float("%.3g" % v) for k, v in report.items()})
    bad = unit_spy.failures(results)
    assert len(results) > 8 and not bad, bad


@pytest.mark.parametrize("case", UNIT_CASES, ids=[f"{n}-w{2 * w}-{d}" for n, w, d in UNIT_CASES])
def test_resize_units_against_float64(sg, case):
    """d1: input (1,2,w,256) -> conv on (1,4,2w,256); d2: (1,2,w,128) -> (1,4,2w,128), at ngf 64, w = 64 (conv grid 128 wide: HALO3 in
    bf16) and w = 32 (64 wide: the generic GEMM), single unit and lockstep pair, against the float64 unit with its derived bounds."""
    name, w_in, dtype = case
    mode = "bilinear" if name == "d1" else "nearest"
    route = "HALO3" if (dtype == "bf16" and w_in == 64) else "GLDS"
    Ga = sg.Generator(gf_dim=64, n_blocks=1, dtype=DT[dtype], upsample=mode, seed=31)
    Gb = sg.Generator(gf_dim=64, n_blocks=1, dtype=DT[dtype], upsample=mode, seed=32)
    assert getattr(Ga, name).kind == "conv" and getattr(Ga, name).padding == "SAME" and getattr(Ga, name).stride == 1
    h, dy = _unit_inputs(name, w_in, dtype, 1, 5)
    _check_unit(sg, getattr(Ga, name), h, dy, dtype, mode, route)
    h2, dy2 = _unit_inputs(name, w_in, dtype, 2, 6)
    _check_unit(sg, sg.module._PairUnit(getattr(Ga, name), getattr(Gb, name)), h2, dy2, dtype, mode, route)


# ----------------------------------------------------------------------------- 5. the generator
def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _gen_params(rng, ngf, n_blocks):
    return {k: _f32(v) for k, v in O.init_params(UO.generator_param_shapes(ngf, 3, 3, n_blocks), rng, 0.1).items()}


def _pos(t, c, sl=slice(None)):
    return (t[sl][..., :c] > 0).cpu().numpy()


def resize_generator_branches(sg, G, tape, params, sl=slice(None)):
    """tests/kink_helpers.generator_branches for a resize generator: d1's output is no longer d2's saved input (that is the
    resampled tensor), so its decisions are read from the norm's output recomputed from the record by the unit's own launch
    (bitwise reproducible) -- with the gamma and beta the FORWARD ran on, ``params`` (the step's Adam has moved the network's
    since): one parameter dict, or the two of a lockstep pair's stacked tape."""
    K, A = sg.kernels, sg._abi
    nb = G.n_blocks
    out = [_pos(tape[1][1], G.c1.cout, sl), _pos(tape[2][1], G.c2.cout, sl), _pos(tape[3][0][1], G.c3.cout, sl)]
    for i in range(nb):
        out.append(_pos(tape[3 + i][1][1], G.blocks[i][0].cout, sl))
    xc = tape[3 + nb][2]
    vec = lambda v: F.pad(torch.as_tensor(np.asarray(v, np.float32)), (0, K.cpad(len(v)) - len(v))).cuda()
    aff = [(vec(P["d1_g"]), vec(P["d1_beta"])) for P in (params if isinstance(params, (list, tuple)) else [params])]
    pair = None if len(aff) == 1 else (aff[1][0], aff[1][1], xc.shape[0] // 2)
    y = K.instnorm_forward(xc, aff[0][0], aff[0][1], None, G.eps, A.ACT_RELU, 0.0, pair=pair)[0]
    out.append(_pos(y, G.d1.cout, sl))
    out.append(_pos(tape[5 + nb][1], G.d2.cout, sl))
    return out


def _l2(got, exp):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    return float(np.sqrt(((got - exp) ** 2).sum()) / max(np.sqrt((exp ** 2).sum()), 1e-300))


def _rel(got, exp):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    return float(np.abs(got - exp).max() / max(np.abs(exp).max(), 1e-12))


@pytest.mark.parametrize("mode", UO.MODES)
def test_generator_forward_and_backward_against_float64(sg, mode):
    """f32, ngf 8, one block, 2x32x32: the image to 1e-4 of its largest entry, the input gradient and every parameter gradient to
    2e-4 relative L2 of generator_resnet_resize (kink-aware, tests/test_gpu_step.py's figures).  Then GeneratorPair on the stacked
    batch against one network at a time: images and data gradients bitwise, weight gradients to 1e-5 of the tensor norm."""
    K = sg.kernels
    rng = np.random.default_rng(41)
    Pa, Pb = _gen_params(rng, 8, 1), _gen_params(rng, 8, 1)
    xa, xb = _f32(rng.uniform(0, 1, (2, 32, 32, 3))), _f32(rng.uniform(0, 1, (2, 32, 32, 3)))
    dya, dyb = _f32(rng.standard_normal((2, 32, 32, 3))), _f32(rng.standard_normal((2, 32, 32, 3)))
    Ga = sg.Generator(gf_dim=8, n_blocks=1, dtype=torch.float32, upsample=mode, seed=None)
    Gb = sg.Generator(gf_dim=8, n_blocks=1, dtype=torch.float32, upsample=mode, seed=None)
    Ga.P.load(Pa); Gb.P.load(Pb)
    dev = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    inner = lambda G, a: G.to_internal(dev(a))
    single = []
    for G, P, x, dy in ((Ga, Pa, xa, dya), (Gb, Pb, xb, dyb)):
        G.P.zero_grad()
        y, tape = G.forward(inner(G, x))
        dx = G.backward(tape, K.pad_channels(dev(dy), 8, torch.float32), want_dx=True)
        single.append((y.clone(), dx.clone(), G.P.grad.clone()))
        pol = O.KinkPolicy(1e-4, resize_generator_branches(sg, G, tape, P))
        O.KINKS = pol
        try:
            t = O.Tape()
            V, xv = {k: O.Var(v, k) for k, v in P.items()}, O.Var(x)
            out = UO.generator_resnet_resize(t, V, xv, mode, 1)
            t.backward([(out, dy)])
        finally:
            O.KINKS = None
        assert pol.calls == 6 and pol.disagree_outside == 0
        assert _rel(y[..., :3].cpu().numpy(), out.v) < 1e-4
        errs = {"dx": _l2(dx[..., :3].cpu().numpy(), xv.g)}
        for k, v in G.P.export(G.P.grad).items():
            if k.endswith("_b") and k != "out_b":           # a bias in front of an instance norm: exactly 0 here, ~1e-17 in the oracle
                assert np.abs(v).max() == 0.0 and np.abs(V[k].g).max() < 1e-9
                continue
            errs[k] = _l2(v, V[k].g)
        print(f"[{mode}] generator against float64, relative L2:", {k: float("%.1e" % e) for k, e in errs.items()})
        assert max(errs.values()) < 2e-4, errs
    pair = sg.module.GeneratorPair(Ga, Gb)
    Ga.P.zero_grad(); Gb.P.zero_grad()
    y, tape = pair.forward(torch.cat([inner(Ga, xa), inner(Gb, xb)]))
    dx = pair.backward(tape, torch.cat([K.pad_channels(dev(dya), 8, torch.float32), K.pad_channels(dev(dyb), 8, torch.float32)]), want_dx=True)
    for k, (G, (y1, dx1, g1)) in enumerate(zip((Ga, Gb), single)):
        sl = slice(2 * k, 2 * k + 2)
        assert torch.equal(y[sl], y1) and torch.equal(dx[sl], dx1)
        assert float((G.P.grad.double() - g1.double()).norm() / g1.double().norm()) < 1e-5


# ----------------------------------------------------------------------------- 6. the steps against float64
def _step_inputs(rng, N, H, W):
    real = _f32(rng.uniform(0, 1, (N, H, W, 3)))
    pal = rng.integers(0, 256, (8, 3)) / 255.0
    seg = _f32(pal[np.repeat(np.repeat(rng.integers(0, 8, (N, H // 32, W // 32)), 32, 1), 32, 2)])
    mask = np.stack([O.one_hot(i, 34) for i in rng.integers(0, 34, (N, 4, 4))]).astype(np.float64)
    return real, seg, mask


def _disc_params(rng, ndf):
    return {k: _f32(v) for k, v in O.init_params(O.discriminator_param_shapes(df_dim=ndf), rng, 0.1).items()}


def _hold_gradients(nets, exp, label):
    """Every gradient tensor to 2e-4 relative L2 and 2e-4 of its largest entry (tests/test_gpu_step.py's figures and skips)."""
    worst = {}
    for n, net in nets.items():
        got = net.P.export(net.P.grad)
        for k, e in exp[n].items():
            if np.abs(e).max() < 1e-9:                       # biases in front of a norm; D's tail at 128x128 (a 1x1 map): no signal
                assert np.abs(got[k]).max() < 1e-6, (n, k)
                continue
            worst[(n, k)] = (_l2(got[k], e), _rel(got[k], e))
    top = sorted(worst.items(), key=lambda kv: -kv[1][0])[:4]
    print(f"{label}: {len(worst)} gradient tensors, largest errors (relative L2, worst entry):", [(k, "%.1e" % a, "%.1e" % b) for k, (a, b) in top])
    bad = {k: v for k, v in worst.items() if not (v[0] < 2e-4 and v[1] < 2e-4)}
    assert len(worst) > 20 and not bad, bad


@pytest.mark.parametrize("mode", UO.MODES)
def test_reference_step_against_float64(sg, mode):
    """f32, ngf = ndf = 8, one block, 2x128x128: losses to 1e-5, image and logits to 1e-4, every gradient tensor to 2e-4 relative
    L2 of the float64 reference step with the resize generator, evaluated kink-aware."""
    from tests.kink_helpers import discriminator_branches
    rng = np.random.default_rng(43)
    PG, PD = _gen_params(rng, 8, 1), _disc_params(rng, 8)
    real, seg, mask = _step_inputs(rng, 2, 128, 128)
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="f32", keep_tapes=True, upsample=mode))
    m.generator.P.load(PG); m.discriminator.P.load(PD)
    m.real_A, m.seg_A, m.mask_A = real, seg, mask
    m.train_step()
    gl, dl = m.losses()
    t = m.tapes
    branches = (resize_generator_branches(sg, m.generator, t["G"], PG) + discriminator_branches(m.discriminator, t["D_real"])
                + discriminator_branches(m.discriminator, t["D_fake"]))
    pol = O.KinkPolicy(1e-4, branches)
    O.KINKS = pol
    try:
        sp = UO.SignPolicy(1e-4)
        r = UO.train_step(lambda tp, V, x: UO.generator_resnet_resize(tp, V, x, mode, 1), PG, PD, real, seg, mask, signs=sp,
                          device={"fake_A": m.fake_A.numpy()})
    finally:
        O.KINKS = None
    print(f"sign() terms: {sp.ambiguous} arguments within 1e-4 of zero, {sp.overridden} taken with the other sign, {sp.disagree_outside} outside the band")
    assert sp.disagree_outside == 0
    print(f"kink-aware oracle: {pol.elements} activations, {pol.ambiguous} within 1e-4 of a kink, {pol.overridden} taken on the other side, "
          f"{pol.disagree_outside} disagreements outside the band")
    assert pol.calls == len(branches) and pol.disagree_outside == 0
    assert abs(gl - r["gen_loss"]) < 1e-5 * abs(r["gen_loss"]) and abs(dl - r["disc_loss"]) < 1e-5 * abs(r["disc_loss"])
    assert _rel(m.fake_A.numpy(), r["fake_A"]) < 1e-4
    assert _rel(m.da_real.cpu().numpy(), r["da_real"]) < 1e-4 and _rel(m.da_fake.cpu().numpy(), r["da_fake"]) < 1e-4
    _hold_gradients({"G": m.generator, "D": m.discriminator}, {"G": r["gG"], "D": r["gD"]}, f"reference step [{mode}]")


def _cycle_branches(sg, m, P):
    """tests/kink_helpers.cycle_step_branches with the resize generators' decisions."""
    from tests.kink_helpers import discriminator_branches
    t, n = m.tapes, m.tapes["n"]
    lo, hi = slice(0, n), slice(n, 2 * n)
    Gab, Gba, Da, Db = m.generator, m.generator_BA, m.discriminator, m.discriminator_B
    first, second = (P["Gab"], P["Gba"]), (P["Gba"], P["Gab"])          # G_first = (G_ab; G_ba), G_second = (G_ba; G_ab)
    out = (resize_generator_branches(sg, Gab, t["G_first"], first, lo) + resize_generator_branches(sg, Gba, t["G_second"], second, lo)
           + resize_generator_branches(sg, Gba, t["G_first"], first, hi) + resize_generator_branches(sg, Gab, t["G_second"], second, hi))
    q = t["D_quad"]
    return out + (discriminator_branches(Db, q, slice(n, 2 * n)) + discriminator_branches(Da, q, slice(2 * n, 3 * n))
                  + discriminator_branches(Da, q, slice(3 * n, 4 * n)) + discriminator_branches(Db, q, slice(0, n)))


@pytest.mark.parametrize("mode", UO.MODES)
def test_cycle_step_against_float64(sg, mode):
    """The paired cycle step (the default sequencing, d_quad) at the same size against the float64 cycle step with the resize
    generators: losses to 2e-5, images to 1e-4 (the cycled ones 2e-4), every gradient tensor of the four networks to 2e-4.  Beside
    the activations' kinks the sign() of the L1 and gradient-sensitive terms is followed inside the same 1e-4 band
    (tests/upsample_oracle.SignPolicy: without it one image difference within 1e-6 of zero left every generator tensor 2.5e-3 to
    7.8e-3 away, on three of six seeds tried, in either mode)."""
    rng = np.random.default_rng(47)
    P = {"Gab": _gen_params(rng, 8, 1), "Gba": _gen_params(rng, 8, 1), "Da": _disc_params(rng, 8), "Db": _disc_params(rng, 8)}
    (real_A, seg_A, mask_A), (real_B, seg_B, mask_B) = _step_inputs(rng, 2, 128, 128), _step_inputs(rng, 2, 128, 128)
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="f32", cycle=True, keep_tapes=True, upsample=mode))
    assert m.paired and m.d_quad
    nets = {"Gab": m.generator, "Gba": m.generator_BA, "Da": m.discriminator, "Db": m.discriminator_B}
    for n, net in nets.items():
        net.P.load(P[n])
    m.real_A, m.real_B, m.seg_A, m.seg_B, m.mask_A, m.mask_B = real_A, real_B, seg_A, seg_B, mask_A, mask_B
    m.train_step()
    gl, dl = m.losses()
    branches = _cycle_branches(sg, m, P)
    pol, sp = O.KinkPolicy(1e-4, branches), UO.SignPolicy(1e-4)
    O.KINKS = pol
    try:
        r = UO.cycle_step(lambda tp, V, x: UO.generator_resnet_resize(tp, V, x, mode, 1), P["Gab"], P["Gba"], P["Da"], P["Db"],
                          real_A, real_B, seg_A, seg_B, mask_A, mask_B, signs=sp,
                          device={k: getattr(m, k).numpy() for k in ("fake_A", "fake_B", "cyc_A", "cyc_B")})
    finally:
        O.KINKS = None
    print(f"kink-aware oracle: {pol.elements} activations, {pol.ambiguous} within 1e-4 of a kink, {pol.overridden} taken on the other side, "
          f"{pol.disagree_outside} disagreements outside the band")
    print(f"sign() terms: {sp.ambiguous} arguments within 1e-4 of zero, {sp.overridden} taken with the other sign, {sp.disagree_outside} outside the band")
    assert pol.calls == len(branches) and pol.disagree_outside == 0 and sp.disagree_outside == 0
    assert abs(gl - r["g_loss"]) < 2e-5 * abs(r["g_loss"]) and abs(dl - r["d_loss"]) < 2e-5 * abs(r["d_loss"]), (gl, r["g_loss"], dl, r["d_loss"])
    assert _rel(m.fake_B.numpy(), r["fake_B"]) < 1e-4 and _rel(m.cyc_A.numpy(), r["cyc_A"]) < 2e-4
    assert _rel(m.fake_A.numpy(), r["fake_A"]) < 1e-4 and _rel(m.cyc_B.numpy(), r["cyc_B"]) < 2e-4
    _hold_gradients(nets, r["grads"], f"cycle step [{mode}]")


# ----------------------------------------------------------------------------- 7. bitwise identities
def _model(sg, seed_inputs=61, N=2, H=128, W=128, **kw):
    from tests.test_gpu_step import _rand_inputs
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=2, **kw))
    m.real_A, m.seg_A, m.mask_A = _rand_inputs(N, H, W, m.discriminator, seed_inputs)
    if m.cycle:
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(N, H, W, m.discriminator, seed_inputs + 1)
    return m


def _state(m):
    imgs = [m.fake_A.tensor()] + ([m.fake_B.tensor(), m.cyc_A.tensor(), m.cyc_B.tensor()] if m.cycle else [])
    return [t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.grad)] + [m._loss.clone()] + [t.clone() for t in imgs]


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", UO.MODES)
def test_graph_replay_equals_eager(sg, mode, dtype, cycle):
    out = []
    for graph in (False, True):
        m = _model(sg, dtype=dtype, cycle=cycle, upsample=mode, graph=graph)
        for _ in range(2):
            m.train_step()
        out.append(_state(m))
    for k, (a, b) in enumerate(zip(*out)):
        assert torch.equal(a, b), ("tensor", k)


OPTIONS = {"guards": dict(clip_grad_norm=1.0, skip_nonfinite=True), "diffaug": dict(diffaug="color,cutout"), "ssim": dict(ssim_lambda=1.0),
           "spectral": dict(d_norm="spectral"), "pool": dict(use_pool=True), "ema": dict(ema_decay=0.9), "mixed": dict(mixed=True)}


COMPOSED = [(o, c) for o in sorted(OPTIONS) for c in (False, True) if c or o != "pool"]       # (the image pool belongs to the cycle step)


@pytest.mark.parametrize("option,cycle", COMPOSED, ids=[f"{o}-{'cycle' if c else 'reference'}" for o, c in COMPOSED])
def test_graph_replay_equals_eager_beside_each_other_option(sg, option, cycle):
    """bilinear, bf16: the resampling has no state, so beside every other option of the step a replayed step is still the eager one
    bit for bit, with finite losses (the pool only exists in the cycle step, where it takes the static form under replay)."""
    out = []
    for graph in (False, True):
        kw = dict(OPTIONS[option], pool_static=True) if option == "pool" else OPTIONS[option]
        m = _model(sg, dtype="bf16", cycle=cycle, upsample="bilinear", graph=graph, **kw)
        for _ in range(2):
            m.train_step()
        assert all(np.isfinite(v) for v in m.losses())
        out.append(_state(m))
    for k, (a, b) in enumerate(zip(*out)):
        assert torch.equal(a, b), ("tensor", k)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", UO.MODES)
def test_paired_cycle_step_equals_one_network_at_a_time(sg, mode, dtype):
    """As tests/test_gpu_step.py states it for the transposed network (d_quad off): losses, images and data gradients bitwise;
    buffers that hold weight gradients of layers whose two networks share a launch to 1e-5 of their norm."""
    out = []
    for paired in (False, True):
        m = _model(sg, dtype=dtype, cycle=True, upsample=mode, paired=paired, d_quad=False)
        m.train_step()
        out.append(_state(m))
    nbuf = 4 * 4
    for k, (a, b) in enumerate(zip(*out)):
        if torch.equal(a, b):
            continue
        assert k < nbuf, ("tensor", k)
        assert float((a.double() - b.double()).norm() / b.double().norm()) < 1e-5, ("tensor", k)


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
@pytest.mark.parametrize("mode", UO.MODES)
def test_save_load_resumes_bitwise(sg, mode, cycle, tmp_path):
    a = _model(sg, dtype="bf16", cycle=cycle, upsample=mode)
    a.train_step(); a.train_step()
    b = _model(sg, dtype="bf16", cycle=cycle, upsample=mode)
    b.train_step()
    b.save(str(tmp_path), 0)
    c = _model(sg, dtype="bf16", cycle=cycle, upsample=mode, seed=77)
    assert c.load(str(tmp_path))
    c.train_step()
    for k, (x, y) in enumerate(zip(_state(a), _state(c))):
        assert torch.equal(x, y), ("tensor", k)


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
@pytest.mark.parametrize("mode", UO.MODES)
def test_checkpoint_blocks_changes_no_bit(sg, mode, cycle):
    out = []
    for ckpt in (False, True):
        m = _model(sg, dtype="bf16", cycle=cycle, upsample=mode, checkpoint_blocks=ckpt)
        assert m.generator.checkpoint_blocks == ckpt
        for _ in range(2):
            m.train_step()
        out.append(_state(m))
    for k, (a, b) in enumerate(zip(*out)):
        assert torch.equal(a, b), ("tensor", k)


# ----------------------------------------------------------------------------- 8. checkpoint tags
def test_checkpoint_tags(sg):
    models = {u: sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, cycle=True, upsample=u)) for u in ("deconv", "nearest", "bilinear")}
    sds = {u: m.state_dict() for u, m in models.items()}
    # option off: the parent's key sets
    assert set(sds["deconv"]) == {"G", "D", "G_BA", "D_B"}
    assert set(sds["deconv"]["G"]) == {"flat", "m", "v", "t", "arch"} and set(sds["deconv"]["G_BA"]) == {"flat", "m", "v", "t"}
    assert set(sds["deconv"]["D"]) == set(sds["deconv"]["D_B"]) == {"flat", "m", "v", "t"}
    ref = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1)).state_dict()
    assert set(ref) == {"G", "D"} and set(ref["G"]) == {"flat", "m", "v", "t", "arch"}
    for u in UO.MODES:
        assert sds[u]["G"]["upsample"] == u and sds[u]["G_BA"]["upsample"] == u and "upsample" not in sds[u]["D"]
        assert sds[u]["G"]["flat"].numel() == sds["deconv"]["G"]["flat"].numel()
    for src in sds:
        for dst, m in models.items():
            if src == dst:
                m.load_state_dict(sds[src])
                continue
            with pytest.raises(ValueError, match=f"--upsample {src}"):      # (names the flag to use)
                m.load_state_dict(sds[src])
    untagged = {k: {f: v for f, v in d.items() if f != "upsample"} for k, d in sds["nearest"].items()}
    models["deconv"].load_state_dict(untagged)                               # a missing tag means deconv
    with pytest.raises(ValueError, match="--upsample deconv"):
        models["bilinear"].load_state_dict(untagged)


# ----------------------------------------------------------------------------- 9. launches
# The default model's captured launches at 2 x 128 x 128, bf16, ngf = ndf = 8, n_blocks = 1, counted by tests/test_gpu_spectral.py's
# procedure (spectral_off_counts) on a checkout of the parent commit fa877fa: the constants that file already pins.
def test_option_off_launch_counts_are_the_parents(sg):
    from tests.test_gpu_spectral import PARENT_NODES, spectral_off_counts
    assert PARENT_NODES == {"D": 60, "reference": 176, "cycle": 319}
    got = spectral_off_counts(sg)
    print("captured launches, option off:", got)
    assert got == PARENT_NODES


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
@pytest.mark.parametrize("mode", UO.MODES)
def test_option_on_launches(sg, mode, cycle, monkeypatch):
    """The option-on step's captured launches are printed (a conv unit and a transposed unit need not launch alike); what is fixed:
    per resize layer and application of a network exactly one resampling and one adjoint launch -- the paired cycle step applies
    the two generators as two stacked passes, so 2 layers x 2 passes; the reference step 2 layers x 1."""
    from tests.test_gpu_spectral import _captured_nodes
    K = sg.kernels
    from tests.test_gpu_step import _rand_inputs
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=cycle, upsample=mode))
    m.real_A, m.seg_A, m.mask_A = _rand_inputs(2, 128, 128, m.discriminator, 40)
    if cycle:
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(2, 128, 128, m.discriminator, 50)
    m.train_step()
    m._stage_inputs()
    torch.cuda.synchronize()
    calls = {"fwd": [], "bwd": []}
    lib = sg._abi.lib()
    real_f, real_b = lib.sgg_upsample2x_fwd, lib.sgg_upsample2x_bwd
    monkeypatch.setattr(K, "upsample2x", (lambda f: lambda x, md, out=None: (calls["fwd"].append(tuple(x.shape)), f(x, md, out))[1])(K.upsample2x))
    monkeypatch.setattr(K, "upsample2x_bwd", (lambda f: lambda dy, md, out=None: (calls["bwd"].append(tuple(dy.shape)), f(dy, md, out))[1])(K.upsample2x_bwd))
    nodes = _captured_nodes(m.device, m._step_body)
    print(f"captured launches, --upsample {mode}, {'cycle' if cycle else 'reference'} step: {nodes}")
    apps, n = (2, 4) if cycle else (1, 2)
    want_f = [(n, 32, 32, 32), (n, 64, 64, 16)] * apps               # d1's input at ngf 8: 4*ngf channels at H/4; d2's: 2*ngf at H/2
    want_b = [(n, 128, 128, 16), (n, 64, 64, 32)] * apps             # the adjoints, in backward order: d2's then d1's
    assert calls["fwd"] == want_f and calls["bwd"] == want_b, calls
    assert real_f is lib.sgg_upsample2x_fwd and real_b is lib.sgg_upsample2x_bwd


# ----------------------------------------------------------------------------- 10. the weight average
@pytest.mark.parametrize("mode", UO.MODES)
def test_ema_with_the_option(sg, mode):
    """--ema_decay with a resize generator: ema_weights() swaps the average in and out bit for bit; inside the context generator(x)
    is the RESIZE network on the averaged weights (held to the float64 generator_resnet_resize); and the test pass returns the
    images of that network, computed here by hand as tests/test_gpu_ema.py does."""
    from sggan_amd.main import parse_args, synthetic_test_samples
    from sggan_amd.utils import convert_image_dtype_uint8, get_img
    from tests.test_gpu_step import _rand_inputs
    a = parse_args(["--img_height", "128", "--img_width", "128", "--ngf", "8", "--ndf", "8", "--batch_size", "1", "--dtype", "f32",
                    "--upsample", mode, "--ema_decay", "0.9"])
    a.n_blocks, a.test_dir = 1, None
    m = sg.sggan(a)
    assert m.upsample == mode and m.generator.upsample == mode
    m.real_A, m.seg_A, m.mask_A = _rand_inputs(1, 128, 128, m.discriminator, 71)
    for _ in range(2):
        m.train_step()
    G = m.generator
    flat, ema = G.P.flat.clone(), G.P.ema.clone()
    assert not torch.equal(flat, ema)
    x = torch.as_tensor(m.real_A)[:1, :32, :32].contiguous()
    plain = G(x.cuda()).cpu().numpy()
    with m.ema_weights():
        assert torch.equal(G.P.flat, ema) and torch.equal(G.P.ema, flat)
        avg = G(x.cuda()).cpu().numpy()
        P = {k: v.astype(np.float64) for k, v in G.P.export().items()}
    assert torch.equal(G.P.flat, flat) and torch.equal(G.P.ema, ema)
    assert np.array_equal(G(x.cuda()).cpu().numpy(), plain) and not np.array_equal(avg, plain)
    t = O.Tape()
    out = UO.generator_resnet_resize(t, {k: O.Var(v, k) for k, v in P.items()}, O.Var(x.numpy().astype(np.float64)), mode, 1)
    assert _rel(avg, out.v) < 1e-4
    by_hand = lambda: np.concatenate([get_img(G(torch.as_tensor(convert_image_dtype_uint8(np.asarray(s[1])[None])).to(m.device)), [1, 1])
                                      for s in synthetic_test_samples(a, 1)()], axis=0)
    images, _ = m.test_during_train(0, a, synthetic_test_samples(a, 1)())
    with m.ema_weights():
        want = by_hand()
    assert np.array_equal(images, want) and not np.array_equal(want, by_hand())
    assert torch.equal(G.P.flat, flat) and torch.equal(G.P.ema, ema)
