"""Spectral-norm discriminators (--d_norm spectral) on the GPU: the three kernels against the float64 oracle
(tests/spectral_oracle.py) at their band, chunk and fold edges, the network and the steps against the composed oracle, graph
replay, resume, the combinations, and the option switched off."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sggan_oracle as O
from tests import spectral_oracle as S

pytestmark = pytest.mark.gpu

# the kernels' constants (csrc/spectral.hip): a block takes BAND rows, its WAVES waves one row each, two rounds at a time; a lane
# owns LANES * V consecutive-chunk columns (V = 4 floats per 16-byte load where K % 4 == 0, else 1), in 1, 2, 4 (8, 16) chunks;
# a fold block takes FOLD columns, and THREADS bands (or rows) at a time
BAND, WAVES, LANES, FOLD, THREADS, MAX_K = 32, 4, 64, 64, 256, 1024
SENTINEL = -7.25
U_BOUND = 2.0 ** -22

BASE = [(27, 8), (27, 64), (72, 16), (576, 34)]
ROW_EDGES = [(r, 16) for r in (1, WAVES - 1, WAVES, WAVES + 1, 2 * WAVES - 1, 2 * WAVES, 2 * WAVES + 1,
                               BAND - 1, BAND, BAND + 1, 2 * BAND - 1, 2 * BAND, 2 * BAND + 1)]
COL_EDGES = [(40, k) for k in (1, 3, LANES - 1, LANES + 1, 2 * LANES - 1, 2 * LANES + 1, 4 * LANES + 1, 8 * LANES + 1,      # 4-byte chunks
                               4 * LANES - 4, 4 * LANES, 4 * LANES + 4, 8 * LANES, 8 * LANES + 4,                          # 16-byte chunks
                               THREADS - 1, THREADS + 1, MAX_K - 1, MAX_K)]
FOLD_EDGES = [(THREADS * BAND + 1, 8), (THREADS + 1, 2 * FOLD + 4), (THREADS - 1, FOLD - 4), (2 * THREADS + 1, FOLD)]   # bands / rows / columns per fold block


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


@pytest.fixture(scope="module")
def K():
    from sggan_amd import kernels
    return kernels


def _guarded(n, fill=None):
    """A device f32 buffer of n elements with four sentinel cells behind it: (view, whole)."""
    whole = torch.full((n + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    if fill is not None:
        whole[:n] = torch.as_tensor(fill, dtype=torch.float32).reshape(-1)
    return whole[:n], whole


class _Case:
    """Device buffers of a list of (rows, K) matrices, each with guard cells, and the table over them."""

    def __init__(self, K, shapes, seed, zero=False, grads=None):
        rng = np.random.default_rng(seed)
        self.shapes, self.W, self.u0, self.bufs, entries = shapes, [], [], [], []
        for i, (rows, k) in enumerate(shapes):
            W = np.zeros((rows, k), np.float32) if zero else rng.standard_normal((rows, k)).astype(np.float32)
            u = rng.standard_normal(k)
            u = (u / np.linalg.norm(u)).astype(np.float32)
            w, _ = _guarded(rows * k, W)
            g, gw = _guarded(rows * k, np.zeros(rows * k) if grads is None else grads[i])
            ud, uw = _guarded(k, u)
            vd, vw = _guarded(rows)
            sd, sw = _guarded(1)
            rd, rw = _guarded(1)
            self.W.append(W); self.u0.append(u)
            self.bufs.append(dict(g=g, u=ud, v=vd, sigma=sd, inv=rd, whole=(gw, uw, vw, sw, rw)))
            entries.append((w.view(rows, k), g.view(rows, k), ud, vd, sd, rd))
        self.table = K.SpectralTable(entries, "cuda")

    def host(self, i):
        b = self.bufs[i]
        return {n: b[n].cpu().numpy().copy() for n in ("g", "u", "v", "sigma", "inv")}

    def guards_intact(self):
        return all(bool((w[-4:] == SENTINEL).all()) for b in self.bufs for w in b["whole"])


def _check_sigma(case, advance=True):
    worst = [0.0, 0.0, 0.0]
    for i, (W, u0) in enumerate(zip(case.W, case.u0)):
        u, v, sigma = S.power_iteration(W.astype(np.float64), u0.astype(np.float64), advance)
        h = case.host(i)
        es = abs(float(h["sigma"][0]) - sigma) / sigma                     # (in double: the stored f32 against the oracle's value)
        eu, ev = np.abs(h["u"].astype(np.float64) - u).max(), np.abs(h["v"].astype(np.float64) - v).max()
        print(f"sigma {case.shapes[i]}: rel {es:.2e}, u {eu:.2e}, v {ev:.2e}")
        assert es < 1e-6 and eu <= U_BOUND and ev <= U_BOUND, (case.shapes[i], es, eu, ev)
        assert abs(float(h["inv"][0]) * sigma - 1) < 2e-7
        if not advance:
            assert np.array_equal(h["u"], u0)
        worst = [max(a, b) for a, b in zip(worst, (es, eu, ev))]
    return worst


# ---- 1. sgg_spectral_sigma ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + ROW_EDGES + COL_EDGES + FOLD_EDGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sigma_matches_the_oracle(K, shape):
    case = _Case(K, [shape], seed=shape[0] * 1031 + shape[1])
    K.spectral_sigma(case.table)
    _check_sigma(case)
    assert case.guards_intact()


def test_sigma_largest_layer_mixed_table_repeat_and_no_advance(K):
    shapes = [(4608, 512), (27, 8), (576, 34), (BAND + 1, 2 * LANES + 1), (72, 16), (1, 1), (2 * BAND, 4 * LANES + 4)]
    case = _Case(K, shapes, seed=77)
    K.spectral_sigma(case.table)
    worst = _check_sigma(case)
    print("largest errors observed (sigma relative, u, v absolute): %.2e %.2e %.2e" % tuple(worst))
    first = [case.host(i) for i in range(len(shapes))]
    for b, u in zip(case.bufs, case.u0):                      # the same inputs again: the same bits
        b["u"].copy_(torch.as_tensor(u))
    K.spectral_sigma(case.table)
    for i, a in enumerate(first):
        b = case.host(i)
        assert all(np.array_equal(a[n], b[n]) for n in ("u", "v", "sigma", "inv")), shapes[i]
    for b, u in zip(case.bufs, case.u0):                      # without advancing: u stays, sigma = |M u|
        b["u"].copy_(torch.as_tensor(u))
    K.spectral_sigma(case.table, advance=False)
    _check_sigma(case, advance=False)
    assert case.guards_intact()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_zero_kernel_gives_finite_outputs_and_a_finite_pack(K, dtype):
    case = _Case(K, [(27, 8), (72, 16)], seed=1, zero=True)
    K.spectral_sigma(case.table)
    for i in range(2):
        h = case.host(i)
        assert h["sigma"][0] == np.float32(1e-12) and h["inv"][0] == np.float32(1e12)
        assert np.all(h["u"] == 0) and np.all(h["v"] == 0)
    w = torch.zeros((3, 3, 3, 8), device="cuda")
    table, n, max_elems, bufs = K.pack_weights_batch([(w, 8, 8, True, True)], dtype, "cuda")
    K.repack_batch(table, n, max_elems, dtype, scale=case.bufs[0]["inv"])
    assert all(bool(torch.isfinite(t.float()).all()) and float(t.float().abs().max()) == 0.0 for t in bufs[0])
    assert case.guards_intact()


# ---- 2. the scaled pack --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shapes", [[(3, 3, 3, 8)], [(3, 3, 64, 34)], [(3, 3, 3, 8), (3, 3, 8, 16), (3, 3, 64, 34), (3, 3, 72, 72)]],
                         ids=["c3", "k34", "mixed"])
def test_scaled_pack_equals_the_plain_pack_of_the_scaled_kernel(K, shapes, dtype):
    g = torch.Generator().manual_seed(len(shapes))
    ws = [torch.randn(s, generator=g).cuda() for s in shapes]
    scale = (torch.rand(len(shapes), generator=g) * 3 + 0.01).cuda()

    def packed(kernels, sc):
        table, n, max_elems, bufs = K.pack_weights_batch([(w, K.cpad(w.shape[2]), K.cpad(w.shape[3]), True, True) for w in kernels], dtype, "cuda")
        for wf, wd in bufs:
            wf.fill_(SENTINEL); wd.fill_(SENTINEL)
        K.repack_batch(table, n, max_elems, dtype, scale=sc)
        return bufs
    want = packed([w * s for w, s in zip(ws, scale)], None)     # torch forms w * inv_sigma in f32; the existing pack rounds it once
    got = packed(ws, scale)
    ones, plain = packed(ws, torch.ones_like(scale)), packed(ws, None)
    for i in range(len(shapes)):
        for layout in (0, 1):
            assert torch.equal(got[i][layout].view(torch.uint8), want[i][layout].view(torch.uint8)), (shapes[i], layout)
            assert torch.equal(ones[i][layout].view(torch.uint8), plain[i][layout].view(torch.uint8)), (shapes[i], layout)


# ---- 3. sgg_spectral_grad ------------------------------------------------------------------------------------------------------
GRAD_SHAPES = BASE + FOLD_EDGES[:1] + [(BAND - 1, 16), (BAND, 16), (BAND + 1, 16), (2 * BAND + 1, 16), (WAVES + 1, 16), (40, LANES + 1), (40, 4 * LANES),
                      (40, 4 * LANES + 4), (40, 8 * LANES + 1), (40, MAX_K)]


@pytest.mark.parametrize("kind", ["dyadic", "random"])
@pytest.mark.parametrize("shapes", [[s] for s in GRAD_SHAPES] + [[(4608, 512), (27, 8), (576, 34), (72, 16)]],
                         ids=lambda ss: "+".join(f"{r}x{k}" for r, k in ss))
def test_grad_transform_matches_the_oracle(K, shapes, kind):
    rng = np.random.default_rng(sum(r * 7 + k for r, k in shapes))
    if kind == "dyadic":
        grads = [(rng.integers(-64, 65, (r, k)) / 32.0).astype(np.float32) for r, k in shapes]
    else:
        grads = [rng.standard_normal((r, k)).astype(np.float32) for r, k in shapes]
    case = _Case(K, shapes, seed=5, grads=grads)
    K.spectral_sigma(case.table)
    K.spectral_grad(case.table)
    out = [case.host(i) for i in range(len(shapes))]
    for i, (W, G) in enumerate(zip(case.W, grads)):
        h = out[i]
        f64 = lambda a: np.asarray(a, np.float64)
        exp = S.grad_transform(f64(G), f64(W), f64(h["u"]), f64(h["v"]), float(h["inv"][0])).astype(np.float32)
        got = h["g"].reshape(W.shape)
        ulp = np.spacing(np.abs(exp))
        assert np.all(np.abs(got - exp) <= ulp), (shapes[i], float(np.abs(got - exp).max()))
        dot = abs(float((f64(got) * f64(W)).sum()))
        assert dot <= 1e-5 * np.linalg.norm(f64(got)) * np.linalg.norm(f64(W)), (shapes[i], dot)
    for b, G in zip(case.bufs, grads):                        # the same inputs again: the same bits
        b["g"].copy_(torch.as_tensor(G).reshape(-1))
    K.spectral_grad(case.table)
    for i in range(len(shapes)):
        assert np.array_equal(case.host(i)["g"], out[i]["g"])
    assert case.guards_intact()


# ---- 4. the network ------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _d_params(rng, ndf=8):
    shapes = S.discriminator_param_shapes(df_dim=ndf)
    return {k: _f32(v) for k, v in O.init_params(shapes, rng, 0.1).items()}


def _u_of(D):
    return {n: v[0].astype(np.float64) for n, v in D.spectral_vectors().items()}


def _worst(got, exp):
    out = {}
    for k, e in exp.items():
        if np.abs(e).max() < 1e-9:
            continue
        d = np.asarray(got[k], np.float64) - e
        out[k] = (float(np.sqrt((d ** 2).sum()) / np.sqrt((e ** 2).sum())), float(np.abs(d).max() / np.abs(e).max()))
    return out


def test_spectral_discriminator_forward_backward_and_autograd_match_the_oracle(sg):
    from tests.kink_helpers import discriminator_branches
    rng = np.random.default_rng(31)
    PD = _d_params(rng)
    D = sg.Discriminator(df_dim=8, dtype=torch.float32, norm="spectral", seed=4)
    assert D.P.names() == [n for n, _ in S.discriminator_param_shapes(df_dim=8)] and all(not u.norm for u in D.conv_units())
    D.P.load(PD)
    U0 = _u_of(D)
    x, mask = _f32(rng.uniform(0, 1, (2, 128, 128, 3))), np.stack([O.one_hot(i, 34) for i in rng.integers(0, 34, (2, 1, 1))]).astype(np.float64)
    dlog = _f32(rng.standard_normal((2, 1, 1, 1)))
    assert D.out_hw(128, 128) == (1, 1)
    xd, md, dd = (torch.as_tensor(a, dtype=torch.float32).cuda() for a in (x, mask, dlog))
    logits, tape = D.forward(D.to_internal(xd), md)
    u_bits = D.spectral_state().clone()
    D.P.zero_grad()
    dx = D.backward(tape, dd, want_dx=True)
    D.spectral_grad()
    pol = O.KinkPolicy(1e-4, discriminator_branches(D, tape))
    O.KINKS = pol
    try:
        r = S.discriminator_grads(PD, U0, x, mask, dlog)
    finally:
        O.KINKS = None
    assert pol.disagree_outside == 0
    rel = lambda a, b: np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max()
    assert rel(logits.cpu().numpy(), r["logits"]) < 2e-4
    assert rel(dx[..., :3].cpu().numpy(), r["dx"]) < 2e-4                    # the image gradient, what the generators receive
    sv = D.spectral_vectors()
    assert all(abs(sv[n][2] - r["sigma"][n]) < 1e-6 * r["sigma"][n] for n in S.LAYERS)
    w1 = _worst(D.P.export(D.P.grad), r["grads"])
    print("spectral D, forward/backward: worst", sorted(w1.items(), key=lambda kv: -kv[1][0])[:3])
    assert len(w1) == 16 and all(a < 2e-4 and b < 2e-4 for a, b in w1.values()), w1
    # the autograd facade: gradients with respect to the stored variables
    D.requires_grad_(True)
    y = D([xd, md])
    y.backward(dd)
    got = {n: v.grad.cpu().numpy() for n, v in zip(D.P.names(), D.trainable_variables)}
    D.requires_grad_(False)
    w2 = _worst(got, r["grads"])
    assert len(w2) == 16 and all(a < 2e-4 and b < 2e-4 for a, b in w2.values()), w2
    # eval forwards do not advance u
    D([xd, md]); D([xd, md])
    assert torch.equal(D.spectral_state(), u_bits)


# ---- 5. the steps ----------------------------------------------------------------------------------------------------------------
def _step_inputs(rng, N=1, H=128, W=128):
    img = lambda: _f32(rng.uniform(0, 1, (N, H, W, 3)))
    pal = rng.integers(0, 256, (8, 3)) / 255.0
    seg = lambda: _f32(pal[np.repeat(np.repeat(rng.integers(0, 8, (N, H // 32, W // 32)), 32, 1), 32, 2)])
    mk = lambda: np.stack([O.one_hot(i, 34) for i in rng.integers(0, 34, (N, 1, 1))]).astype(np.float64)
    return img, seg, mk


def _kinked(branches, fn):
    pol = O.KinkPolicy(1e-4, branches)
    O.KINKS = pol
    try:
        r = fn()
    finally:
        O.KINKS = None
    assert pol.calls == len(branches) and pol.disagree_outside == 0
    return r


@pytest.mark.parametrize("d_quad", [False, True], ids=["two_passes", "d_quad"])
def test_reference_step_two_steps_match_the_oracle(sg, d_quad):
    from tests.kink_helpers import discriminator_branches, generator_branches
    rng = np.random.default_rng(41)
    img, seg, mk = _step_inputs(rng)
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="f32", keep_tapes=True, d_quad=d_quad, d_norm="spectral"))
    PG = {k: _f32(v) for k, v in O.init_params(O.generator_param_shapes(gf_dim=8, n_blocks=1), rng, 0.1).items()}
    m.generator.P.load(PG); m.discriminator.P.load(_d_params(rng))
    G_, D_ = m.generator, m.discriminator
    for step in range(2):                                   # step 2 consumes the u step 1 left
        PG, PD = ({k: v.astype(np.float64) for k, v in net.P.export().items()} for net in (G_, D_))
        U = _u_of(D_)
        real, sg_, mask = img(), seg(), mk()
        m.real_A, m.seg_A, m.mask_A = real, sg_, mask
        m.train_step()
        gl, dl = m.losses()
        t = m.tapes
        br = generator_branches(G_, t["G"]) + discriminator_branches(D_, t["D_real"]) + discriminator_branches(D_, t["D_fake"])
        r = _kinked(br, lambda: S.train_step(PG, PD, U, real, sg_, mask, n_blocks=1))
        assert abs(gl - r["gen_loss"]) < 2e-5 * abs(r["gen_loss"]) and abs(dl - r["disc_loss"]) < 2e-5 * abs(r["disc_loss"]), (step, gl, dl)
        U1 = _u_of(D_)
        assert all(np.abs(U1[n] - r["U"][n]).max() <= U_BOUND for n in S.LAYERS), step
        assert any(np.abs(U1[n] - U[n]).max() > 1e-3 for n in S.LAYERS)                # (u really moved)
        w = {**{("D", k): v for k, v in _worst(D_.P.export(D_.P.grad), r["gD"]).items()},
             **{("G", k): v for k, v in _worst(G_.P.export(G_.P.grad), r["gG"]).items()}}
        print(f"reference step {step + 1} [d_quad={d_quad}]: worst", sorted(w.items(), key=lambda kv: -kv[1][0])[:3])
        assert sum(k[0] == "D" for k in w) == 16                                       # every D tensor, the biases included
        assert all(a < 2e-4 and b < 2e-4 for a, b in w.values()), {k: v for k, v in w.items() if max(v) >= 2e-4}


@pytest.mark.parametrize("cfg", [(True, True), (True, False), (False, True)], ids=["paired-d_quad", "paired-two_passes", "unpaired"])
def test_cycle_step_two_steps_match_the_oracle(sg, cfg):
    from tests.kink_helpers import cycle_step_branches
    paired, d_quad = cfg
    rng = np.random.default_rng(43)
    img, seg, mk = _step_inputs(rng)
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="f32", cycle=True, keep_tapes=paired, d_quad=d_quad, paired=paired,
                                 d_norm="spectral"))
    nets = {"Gab": m.generator, "Gba": m.generator_BA, "Da": m.discriminator, "Db": m.discriminator_B}
    gs = O.generator_param_shapes(gf_dim=8, n_blocks=1)
    for n, net in nets.items():
        net.P.load(_d_params(rng) if n[0] == "D" else {k: _f32(v) for k, v in O.init_params(gs, rng, 0.1).items()})
    # the one-network-at-a-time step keeps no forward records: the kink decisions are read from a lockstep twin that takes the same
    # step from the same parameters and u (its activations are the same bits: tests/test_gpu_step.py pins that)
    twin = m if paired else sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="f32", cycle=True, keep_tapes=True, d_quad=False,
                                                     paired=True, d_norm="spectral"))
    tnets = (twin.generator, twin.generator_BA, twin.discriminator, twin.discriminator_B)
    for step in range(2):
        P = {n: {k: v.astype(np.float64) for k, v in net.P.export().items()} for n, net in nets.items()}
        Ua, Ub = _u_of(nets["Da"]), _u_of(nets["Db"])
        rA, rB, sA, sB, mA, mB = img(), img(), seg(), seg(), mk(), mk()
        for mm in {id(m): m, id(twin): twin}.values():
            if mm is not m:
                for net, tn in zip(nets.values(), tnets):
                    tn.P.load(net.P.export())
                    if tn.spectral_state() is not None:
                        tn.set_spectral_state(net.spectral_state())
            mm.real_A, mm.real_B, mm.seg_A, mm.seg_B, mm.mask_A, mm.mask_B = rA, rB, sA, sB, mA, mB
        if twin is not m:
            twin.train_step()
        m.train_step()
        gl, dl = m.losses()
        # sign() arguments of the L1 / gradient-sensitive terms within 1e-4 of zero follow the images the kernels generated
        # (spectral_oracle.SignPolicy: the kink policy's rule; a disagreement outside that band fails)
        sp = S.SignPolicy(1e-4, {k: getattr(m, k).numpy().astype(np.float64) for k in ("fake_A", "fake_B", "cyc_A", "cyc_B")})
        run = lambda: S.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], Ua, Ub, rA, rB, sA, sB, mA, mB, n_blocks=1, signs=sp)
        r = _kinked(cycle_step_branches(twin), run)
        print(f"signs: {sp.ambiguous} of {sp.elements} within 1e-4 of zero, {sp.overridden} taken the other way by the kernels")
        assert sp.disagree_outside == 0 and sp.ambiguous < 1e-3 * sp.elements
        assert abs(gl - r["g_loss"]) < 2e-5 * abs(r["g_loss"]) and abs(dl - r["d_loss"]) < 2e-5 * abs(r["d_loss"]), (step, gl, dl)
        for key, net in (("Ua", nets["Da"]), ("Ub", nets["Db"])):
            U1 = _u_of(net)
            assert all(np.abs(U1[n] - r[key][n]).max() <= U_BOUND for n in S.LAYERS), (step, key)
        w = {(n, k): v for n, net in nets.items() for k, v in _worst(net.P.export(net.P.grad), r["grads"][n]).items()}
        print(f"cycle step {step + 1} [{cfg}]: worst", sorted(w.items(), key=lambda kv: -kv[1][0])[:3])
        assert sum(k[0] in ("Da", "Db") for k in w) == 32
        assert all(a < 2e-4 and b < 2e-4 for a, b in w.values()), {k: v for k, v in w.items() if max(v) >= 2e-4}


def test_bf16_step_is_finite_and_sigma_follows_the_devices_own_weights(sg):
    from tests.test_gpu_step import _rand_inputs
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=True, d_norm="spectral"))
    for step in range(2):
        before = {key: ({k: v.astype(np.float64) for k, v in D.P.export().items()}, _u_of(D))
                  for key, D in (("Da", m.discriminator), ("Db", m.discriminator_B))}
        m.real_A, m.seg_A, m.mask_A = _rand_inputs(2, 128, 128, m.discriminator, 60 + step)
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(2, 128, 128, m.discriminator, 70 + step)
        m.train_step()
        assert all(np.isfinite(v) for v in m.losses())
        for key, D in (("Da", m.discriminator), ("Db", m.discriminator_B)):
            assert bool(torch.isfinite(D.P.flat).all()) and bool(torch.isfinite(D.P.grad).all())
            U1, _, sig = S.iterate(*before[key])
            sv = D.spectral_vectors()
            for n in S.LAYERS:
                assert abs(sv[n][2] - sig[n]) < 1e-6 * sig[n] and np.abs(sv[n][0] - U1[n]).max() <= U_BOUND, (step, key, n)


# ---- 6. graph replay, 7. resume, 8. combinations ---------------------------------------------------------------------------------
def _state(m):
    out = [t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.iterations, n.P.grad)] + [m._loss.clone()]
    return out + [n.spectral_state().clone() for n in m.networks() if n.spectral_state() is not None]


def _run_steps(sg, steps, graph=False, cycle=True, model=None, first=0, **kw):
    from tests.test_gpu_step import _rand_inputs
    m = model if model is not None else sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=cycle, graph=graph,
                                                                 d_norm="spectral", **kw))
    out = []
    for step in range(first, first + steps):
        m.real_A, m.seg_A, m.mask_A = _rand_inputs(2, 128, 128, m.discriminator, 40 + step)
        if cycle:
            m.real_B, m.seg_B, m.mask_B = _rand_inputs(2, 128, 128, m.discriminator, 50 + step)
        m.train_step()
        out.append(_state(m))
    return m, out


def _same(a, b):
    assert len(a) == len(b)
    for step, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for i, (p, q) in enumerate(zip(x, y)):
            assert torch.equal(p, q), (step, i)


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
def test_three_replayed_steps_equal_three_eager_steps(sg, cycle):
    me, eager = _run_steps(sg, 3, graph=False, cycle=cycle)
    mg, graph = _run_steps(sg, 3, graph=True, cycle=cycle)
    nets = 4 if cycle else 2
    assert mg._program is not None and len(eager[0]) == 5 * nets + 1 + nets // 2          # (... the discriminators' u among the state)
    _same(eager, graph)


def test_resume_after_two_steps_equals_four_uninterrupted(sg, tmp_path):
    _, whole = _run_steps(sg, 4)
    m1, _ = _run_steps(sg, 2)
    m1.save(str(tmp_path), 1)
    m2 = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=True, d_norm="spectral", seed=123))
    assert m2.load(str(tmp_path))
    _, rest = _run_steps(sg, 2, model=m2, first=2)
    _same(whole[2:], rest)
    inst = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=True))
    with pytest.raises(ValueError, match="spectral-norm.*instance-norm"):
        inst.load_state_dict(m1.state_dict())
    with pytest.raises(ValueError, match="instance-norm.*spectral-norm"):
        m2.load_state_dict(inst.state_dict())


def test_clip_records_the_norm_of_the_transformed_gradient(sg):
    m, _ = _run_steps(sg, 1, clip_grad_norm=1e-3)
    nets = (("D", m.discriminator), ("D_B", m.discriminator_B))
    before = {key: {n: D.P.p(n + "_w").double().clone() for n in S.LAYERS} for key, D in nets}     # the kernels step 2 differentiates at
    _run_steps(sg, 1, model=m, first=1)
    st = m.grad_stats()
    for key, D in nets:
        norm = float(torch.linalg.vector_norm(D.P.grad.double()))
        assert st[key]["applied"] == 2 and abs(st[key]["norm"] - norm) <= 1e-12 * norm, (key, st[key], norm)
        assert st[key]["clip"] < 1.0
        # ... and that buffer is the transformed one: no component along any kernel
        for n in S.LAYERS:
            g, w = D.P.g(n + "_w").double(), before[key][n]
            assert float(g.norm()) > 0 and abs(float((g * w).sum())) <= 1e-5 * float(g.norm() * w.norm()), (key, n)


@pytest.mark.parametrize("kw", [dict(diffaug="color,cutout"), dict(use_pool=True, pool_static=True, max_size=2)], ids=["diffaug", "use_pool"])
def test_combinations_match_their_graph_twin(sg, kw):
    import random
    mk = lambda: dict(kw, pool_rng=random.Random(5)) if "use_pool" in kw else kw
    _, eager = _run_steps(sg, 3, graph=False, **mk())
    _, graph = _run_steps(sg, 3, graph=True, **mk())
    _same(eager, graph)


# ---- 9. off ----------------------------------------------------------------------------------------------------------------------
def _captured_nodes(device, body):
    """Nodes a recording of ``body`` captures (sgg_stream_capture_nodes, asked before every segment is closed)."""
    from sggan_amd import _abi as A, kernels as Kn
    from sggan_amd.graph import StepProgram

    class Counting(StepProgram):
        nodes = 0

        def _close(self):
            n = C.c_int(0)
            A.check(A.lib().sgg_stream_capture_nodes(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), C.byref(n)), "nodes")
            self.nodes += n.value
            super()._close()

    prog = Counting(device)
    Kn._RECORDER = prog
    try:
        prog.record(body)
    finally:
        Kn._RECORDER = None
    return prog.nodes


# launches of a default model at 2 x 128 x 128, bf16, ngf = ndf = 8, n_blocks = 1, counted with _captured_nodes on the parent commit
# (tools/bench_spectral.py --count, the same procedure, prints them): the discriminator's forward + backward alone, the reference step, the cycle step
PARENT_NODES = {"D": 60, "reference": 176, "cycle": 319}


def spectral_off_counts(sg):
    from tests.test_gpu_step import _rand_inputs
    out = {}
    for cycle in (False, True):
        m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=cycle))
        m.real_A, m.seg_A, m.mask_A = _rand_inputs(2, 128, 128, m.discriminator, 40)
        if cycle:
            m.real_B, m.seg_B, m.mask_B = _rand_inputs(2, 128, 128, m.discriminator, 50)
        m.train_step()
        m._stage_inputs()                        # (device-resident inputs, as a recorded step reads them: no copy inside the capture)
        torch.cuda.synchronize()
        out["cycle" if cycle else "reference"] = _captured_nodes(m.device, m._step_body)
        if not cycle:
            D = m.discriminator
            x, mask = m._prep(m.real_A), m._convert_input("mask_A", m.mask_A)
            d = torch.ones((2, 4, 4, 1), device="cuda")
            one = lambda: D.backward(D.forward(x, mask)[1], d, want_dx=True)
            one()
            torch.cuda.synchronize()
            out["D"] = _captured_nodes(m.device, one)
    return out


def test_default_model_is_untouched(sg):
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=True))
    assert m.d_norm == "instance"
    for D in (m.discriminator, m.discriminator_B):
        assert D.norm == "instance" and D._sn is None and D.spectral_state() is None and D.pack_scale() is None
        assert len(D.P.specs) == 28
    sd = m.state_dict()
    assert set(sd) == {"G", "D", "G_BA", "D_B"}
    assert set(sd["D"]) == set(sd["D_B"]) == {"flat", "m", "v", "t"} and set(sd["G"]) == {"flat", "m", "v", "t", "arch"}
    got = spectral_off_counts(sg)
    print("captured nodes of the default model:", got)
    assert got == PARENT_NODES
