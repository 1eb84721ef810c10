"""GPU tests of the discriminators' differentiable augmentation (--diffaug): the kernels of csrc/diffaug.hip
against the NumPy statement (tests/diffaug_oracle.py) at their chunk and tail edges, the draw kernel's table bit for bit, the
wiring of the option into the train steps (a neutral table is the plain step), the augmented reference step against a float64
restatement, and the equivalences the step keeps with the option on (graph replay, stacked / two-pass discriminators, paired /
one-at-a-time cycle, checkpoint resume)."""
import numpy as np
import pytest
import torch

from oracle import sggan_oracle as O
from tests import diffaug_oracle as DO

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 2048                    # DA_CHUNK of csrc/diffaug.hip (asserted against kernels.DIFFAUG_CHUNK below)
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
# rows x (H, W): a single pixel (no rectangle: ch = cw = 0), an odd size inside one chunk, exactly one chunk, one chunk + 1
# pixel (a second block with a one-pixel tail), several chunks
SHAPES = [(1, 1), (11, 13), (32, 64), (3, 683), (64, 128)]


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


def _to_dev(a, dtype, pad_value=0.0):
    """(rows,H,W,3) float64 -> the internal layout (8 channels); the padded channels carry ``pad_value``."""
    t = torch.full(a.shape[:3] + (8,), pad_value, dtype=torch.float64)
    t[..., :3] = torch.from_numpy(a)
    return t.to(TORCH_DT[dtype]).to(DEV).contiguous()


def _grid_values(rng, shape):
    """Values in [-1, 2] on the 1/64 grid: exactly representable in bf16 (8 significant bits) and f32."""
    return rng.integers(-64, 129, shape).astype(np.float64) / 64.0


def _bf16_round(a):
    return torch.from_numpy(np.asarray(a, np.float64)).to(torch.bfloat16).to(torch.float64).numpy()


def _bf16_ulp(v):
    """The spacing of bf16 (8 significant bits) at |v|; at 0 the smallest normal's."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 2.0 ** (e - 7)


def _check(name, got, exp, dtype):
    """f32: 8 * 2^-24 * max(1, max|oracle|) per element (at most 6 f32 roundings on values of that size, the sums in double);
    bf16: within one bf16 ulp of the rounded oracle value."""
    got = got[..., :3].to(torch.float64).cpu().numpy()
    err = np.abs(got - (exp if dtype == "f32" else _bf16_round(exp)))
    if dtype == "f32":
        bound = 8 * 2.0 ** -24 * max(1.0, float(np.abs(exp).max()))
        print(f"{name} [f32]: max |err| {err.max():.3e}, bound {bound:.3e}")
        assert err.max() <= bound, (name, float(err.max()), bound)
    else:
        ulp = _bf16_ulp(_bf16_round(exp))
        worst = float((err / ulp).max())
        print(f"{name} [bf16]: max |err| / ulp {worst:.3f}")
        assert np.all(err <= ulp), (name, worst, int((err > ulp).sum()))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernels_against_the_numpy_statement(sg, hw, rows, dtype):
    from sggan_amd import kernels as K
    assert K.DIFFAUG_CHUNK == CHUNK and 32 * 64 == CHUNK and 3 * 683 == CHUNK + 1
    H, W = hw
    rng = np.random.default_rng(1000 * H + 10 * W + rows)
    par = DO.param_rows(3, 19, 2, rows, 1, H, W, DO.COLOR | DO.CUTOUT)
    par_d = torch.from_numpy(par).to(DEV)
    x, g, a = (_grid_values(rng, (rows, H, W, 3)) for _ in range(3))
    xd, gd, ad = _to_dev(x, dtype, 7.0), _to_dev(g, dtype, 7.0), _to_dev(a, dtype, 7.0)   # (garbage in the padded channels)
    keep = xd.clone()

    y = K.diffaug(xd, par_d, 3)
    assert torch.equal(xd, keep)                                        # out of place
    _check("forward", y, DO.forward(x, par), dtype)
    assert not y[..., 3:].any()
    if H > 1:                                                           # the rectangle is there, zeros exactly
        inside = np.stack([DO._inside(par[n], H, W) for n in range(rows)])
        assert inside.any() and not y[..., :3][torch.from_numpy(inside).to(DEV)].any()

    dx = K.diffaug_bwd(gd, par_d, 3)
    _check("adjoint", dx, DO.adjoint(g, par), dtype)
    dxa = K.diffaug_bwd(gd, par_d, 3, addend=ad)
    _check("adjoint + addend", dxa, DO.adjoint(g, par, addend=a), dtype)   # joined once
    assert not dx[..., 3:].any() and not dxa[..., 3:].any()

    neutral = torch.from_numpy(np.tile(DO.NEUTRAL, (rows, 1))).to(DEV)
    yn, dn = K.diffaug(xd, neutral, 3), K.diffaug_bwd(gd, neutral, 3)
    assert torch.equal(yn[..., :3], xd[..., :3]) and torch.equal(dn[..., :3], gd[..., :3])
    assert not yn[..., 3:].any() and not dn[..., 3:].any()

    assert torch.equal(K.diffaug(xd, par_d, 3), y) and torch.equal(K.diffaug_bwd(gd, par_d, 3, addend=ad), dxa)   # run to run


def test_autograd_op_is_the_adjoint(sg):
    """ops.diff_augment on an unpadded (N,H,W,3) f32 tensor: value and gradient are the kernels'."""
    rng = np.random.default_rng(3)
    x, g = _grid_values(rng, (2, 11, 13, 3)), _grid_values(rng, (2, 11, 13, 3))
    par = DO.param_rows(1, 19, 0, 2, 0, 11, 13, 3)
    xt = torch.from_numpy(x).float().to(DEV).requires_grad_(True)
    y = sg.diff_augment(xt, torch.from_numpy(par).to(DEV))
    y.backward(torch.from_numpy(g).float().to(DEV))
    assert tuple(y.shape) == (2, 11, 13, 3)
    _check("op forward", y.detach(), DO.forward(x, par), "f32")
    _check("op backward", xt.grad, DO.adjoint(g, par), "f32")


@pytest.mark.parametrize("t", [0, 1, (1 << 32) + 5])
def test_draw_kernel_table_is_the_numpy_table_bit_for_bit(sg, t):
    from sggan_amd import kernels as K
    it = torch.tensor([t], dtype=torch.int64, device=DEV)
    H, W = 11, 14
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for off in (0, 7):
        for stream in (0, 1, 3):                                        # D_A real, D_A fake, D_B fake
            for policy in (1, 2, 3):
                got = K.diffaug_draw(torch.empty((5, 8), device=DEV), it, 19, off, stream, H, W, policy, 0.25).cpu().numpy()
                want = DO.param_rows(t, 19, off, 5, stream, H, W, policy, 0.25)
                assert np.array_equal(bits(got), bits(want)), (t, off, stream, policy, got, want)
    assert np.array_equal(K.diffaug_draw(torch.empty((2, 8), device=DEV), it, 19, 0, 0, H, W, 0).cpu().numpy(), np.tile(DO.NEUTRAL, (2, 1)))
    # keyed by the sample: one batch of 4 == two batches of 2 at offsets 0 and 2
    whole = K.diffaug_draw(torch.empty((4, 8), device=DEV), it, 19, 0, 1, H, W, 3)
    halves = torch.cat([K.diffaug_draw(torch.empty((2, 8), device=DEV), it, 19, o, 1, H, W, 3) for o in (0, 2)])
    assert torch.equal(whole, halves)
    assert int(it.item()) == t                                          # the counter is read, never written


# ----------------------------------------------------------------------------- the train steps
def _rand_inputs(N, H, W, D, seed):
    g = torch.Generator().manual_seed(seed)
    real = torch.rand((N, H, W, 3), generator=g)
    seg = torch.rand((N, H, W, 3), generator=g)
    mh, mw = D.out_hw(H, W)
    mh, mw = (4, 4) if (mh, mw) == (1, 1) else (mh, mw)
    idx = torch.randint(0, 34, (N, mh, mw), generator=g)
    return real, seg, torch.nn.functional.one_hot(idx, 34).float()


def _feed(m, step=0, N=2, H=256, W=256):
    m.real_A, m.seg_A, m.mask_A = _rand_inputs(N, H, W, m.discriminator, 40 + step)
    if m.cycle:
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(N, H, W, m.discriminator, 50 + step)


def _state(m):
    return [t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.iterations, n.P.grad)] + [m._loss.clone()]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "paired_cycle"])
def test_neutral_table_is_the_plain_step(sg, cycle, dtype):
    """The option's launches with every row forced to [0,1,1,0,0,0,0,0] (policy bits 0 at the draw): losses and the
    discriminators' gradients are bitwise those of the plain step; the generators' gradients meet the join in another place (the
    adjoint kernel instead of h0's data-gradient store): in f32 that is the same single add, so they are bitwise equal too; in bf16
    the data gradient is rounded once more in front of the join, and the difference is only printed."""
    kw = dict(ngf=8, ndf=8, n_blocks=1, dtype=dtype, cycle=cycle)
    plain, aug = sg.sggan(sg.default_args(**kw)), sg.sggan(sg.default_args(diffaug="color,cutout", **kw))
    assert aug.diffaug == 3 and plain.diffaug == 0 and (not cycle or aug.paired and aug.d_quad)
    aug._diffaug_bits = 0
    for m in (plain, aug):
        _feed(m)
        m.train_step()
    assert plain.diffaug_params is None
    rows = 8 if cycle else 4
    assert torch.equal(aug.diffaug_params.cpu(), torch.from_numpy(np.tile(DO.NEUTRAL, (rows, 1))))
    assert torch.equal(plain._loss, aug._loss)
    for a, b in zip(plain.networks(), aug.networks()):
        if "Discriminator" in type(a).__name__:
            assert torch.equal(a.P.grad, b.P.grad)
        else:
            bitwise = torch.equal(a.P.grad, b.P.grad)
            worst = 0.0
            for k, v in a.P.export(a.P.grad).items():
                w = b.P.export(b.P.grad)[k]
                nv = float(np.linalg.norm(v))
                if nv > 0:
                    worst = max(worst, float(np.linalg.norm(v.astype(np.float64) - w)) / nv)
                else:
                    assert not w.any(), k
            print(f"generator gradients [{dtype}]: bitwise {bitwise}, worst tensor {worst:.2e} of its norm")
            if dtype == "f32":      # the join is the same single f32 add in another kernel: bitwise (1e-5 of the norm was the fallback bar)
                assert bitwise, worst


def test_reference_step_against_the_float64_restatement(sg):
    """One augmented reference step (f32, policy color,cutout) against oracle.train_step with the transform as one more taped op
    in front of both discriminator passes, fed the device's own parameter table and evaluated kink-aware (tests/kink_helpers.py):
    every gradient tensor within 2e-4 (relative L2 and worst entry / largest entry)."""
    from tests.kink_helpers import discriminator_branches, generator_branches
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="f32", keep_tapes=True, diffaug="color,cutout"))
    G_, D_ = m.generator, m.discriminator
    PG = {k: v.astype(np.float64) for k, v in G_.P.export().items()}
    PD = {k: v.astype(np.float64) for k, v in D_.P.export().items()}
    real, seg, mask = _rand_inputs(2, 256, 256, D_, 7)
    m.real_A, m.seg_A, m.mask_A = real, seg, mask
    m.train_step()
    gl, dl = m.losses()
    par = m.diffaug_params.cpu().numpy()
    want = np.concatenate([DO.param_rows(0, 19, 0, 2, role, 256, 256, 3) for role in (0, 1)])
    assert np.array_equal(par.view(np.uint32), want.view(np.uint32))              # step 0, seed 19, samples 0 and 1, D_A real / fake
    assert len(np.unique(par[:, :3])) == 12 and np.all(par[:, 5:7] == 128)
    t = m.tapes
    branches = generator_branches(G_, t["G"]) + discriminator_branches(D_, t["D_real"]) + discriminator_branches(D_, t["D_fake"])
    pol = O.KinkPolicy(1e-4, branches)
    O.KINKS = pol
    try:
        r = DO.train_step(PG, PD, real.numpy().astype(np.float64), seg.numpy().astype(np.float64), mask.numpy().astype(np.float64), par, n_blocks=1)
    finally:
        O.KINKS = None
    print(f"kink-aware: {pol.elements} activations, {pol.ambiguous} within 1e-4 of a kink, {pol.overridden} taken on the other side, "
          f"{pol.disagree_outside} disagreements outside the band")
    assert pol.calls == len(branches) and pol.disagree_outside == 0
    assert abs(gl - r["gen_loss"]) < 1e-5 * abs(r["gen_loss"]) and abs(dl - r["disc_loss"]) < 1e-5 * abs(r["disc_loss"])
    # the augmentation changed what D saw: the plain oracle's losses are elsewhere
    r0 = O.train_step(PG, PD, real.numpy().astype(np.float64), seg.numpy().astype(np.float64), mask.numpy().astype(np.float64), n_blocks=1)
    assert abs(dl - r0["disc_loss"]) > 1e-3 * abs(r0["disc_loss"])
    l2 = lambda a, b: float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-300))
    worst = {}
    for label, got_all, exp_all, keep in (("gD", D_.P.export(D_.P.grad), r["gD"], ("h0_b", "h4_b")), ("gG", G_.P.export(G_.P.grad), r["gG"], ("out_b",))):
        for k, v in got_all.items():
            e = exp_all[k]
            if k.endswith("_b") and k not in keep:           # bias in front of an InstanceNorm: exactly 0 here, ~1e-16 in float64
                assert np.abs(v).max() == 0.0 and np.abs(e).max() < 1e-9
                continue
            worst[(label, k)] = (l2(v.astype(np.float64), e), float(np.abs(v - e).max() / max(np.abs(e).max(), 1e-300)))
    print("worst tensors (relative L2, worst entry / largest entry):",
          [(k, "%.1e" % a, "%.1e" % b) for k, (a, b) in sorted(worst.items(), key=lambda kv: -kv[1][0])[:5]])
    assert all(a < 2e-4 and b < 2e-4 for a, b in worst.values()), {k: v for k, v in worst.items() if max(v) >= 2e-4}


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
def test_graph_replay_equals_eager_bitwise_with_the_option(sg, cycle):
    """3 steps, bf16: the draw launches are part of the recorded step and read the step counter from device memory, so a replay
    draws what the eager step draws -- and other rows every step."""
    def run(graph):
        m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=cycle, graph=graph, diffaug="color,cutout"))
        out = []
        for step in range(3):
            _feed(m, step)
            m.train_step()
            out.append(_state(m) + [m.fake_A.tensor().clone(), m.diffaug_params.clone()])
        return m, out
    me, eager = run(False)
    mg, graph = run(True)
    assert mg._program is not None and mg._program.n_graphs >= 1
    for step, (a, b) in enumerate(zip(eager, graph)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (step, i)
    tables = [s[-1] for s in graph]
    assert not torch.equal(tables[0], tables[1]) and not torch.equal(tables[1], tables[2])
    n = 2
    if cycle:       # rows [D_B real; D_B fake; D_A fake; D_A real] of the last step (every counter read 2)
        want = np.concatenate([DO.param_rows(2, 19, 0, n, s, 256, 256, 3) for s in (2, 3, 1, 0)])
    else:
        want = np.concatenate([DO.param_rows(2, 19, 0, n, s, 256, 256, 3) for s in (0, 1)])
    assert np.array_equal(tables[2].cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_reference_step_stacked_pass_equals_two_passes_with_the_option(sg):
    """d_quad on against off, the bounds of test_reference_step_stacked_discriminator_pass_equals_two_passes; the same table."""
    out, tables = [], []
    for quad in (False, True):
        m = sg.sggan(sg.default_args(ngf=16, ndf=16, n_blocks=2, dtype="f32", d_quad=quad, diffaug="color,cutout"))
        m.real_A, m.seg_A, m.mask_A = _rand_inputs(2, 256, 256, m.discriminator, 71)
        m.train_step()
        out.append([m._loss.clone()] + [n.P.grad.clone() for n in m.networks()])
        tables.append(m.diffaug_params.clone())
    assert torch.equal(*tables)
    (la, *ga), (lb, *gb) = out
    lrel = float(((la - lb).abs() / lb.abs()).max())
    rels = [float((a.double() - b.double()).norm() / b.double().norm()) for a, b in zip(ga, gb)]
    print("loss rel", lrel, "grad rel", rels)
    assert lrel < 1e-6 and max(rels) < 1e-4, (lrel, rels)


@pytest.mark.parametrize("cfg", [("f32", 16, 2, 2, 256, 256), ("bf16", 64, 2, 1, 256, 512)], ids=["f32_small", "bf16_full_width"])
def test_cycle_step_stacked_pass_equals_two_passes_with_the_option(sg, cfg):
    """The paired cycle step with real draws, d_quad on (ONE pass over [real_B; fake_B | fake_A; real_A], the whole table, the
    adjoint on the middle rows) against d_quad off (fakes and reals augmented from their own table slices): the same table, and
    the bounds of test_stacked_real_and_fake_discriminator_pass_equals_two_passes -- f32: losses to 1e-6, gradients by direction
    to 1e-4 and, where every activation decision agrees, to 1e-5 of their norm (2e-2 otherwise); bf16: losses to 2e-3, gradients
    by direction.  A table row meeting the wrong image row in either form would move every discriminator gradient."""
    from tests.kink_helpers import cycle_step_branches
    dtype, width, blocks, N, H, W = cfg
    out, decisions, tables = [], [], []
    for quad in (False, True):
        m = sg.sggan(sg.default_args(ngf=width, ndf=width, n_blocks=blocks, dtype=dtype, cycle=True, paired=True, d_quad=quad,
                                     keep_tapes=True, diffaug="color,cutout"))
        m.real_A, m.seg_A, m.mask_A = _rand_inputs(N, H, W, m.discriminator, 61)
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(N, H, W, m.discriminator, 62)
        m.train_step()
        assert (m.tapes["D_quad"] is not None) == quad
        out.append([m._loss.clone()] + [n.P.grad.clone() for n in m.networks()])
        decisions.append(cycle_step_branches(m))
        tables.append(m.diffaug_params.clone())
        m.tapes = None
    assert torch.equal(*tables)
    want = np.concatenate([DO.param_rows(0, 19, 0, N, s, H, W, 3) for s in (2, 3, 1, 0)])
    assert np.array_equal(tables[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    flips = sum(int((a != b).sum()) for a, b in zip(*decisions))
    (la, *ga), (lb, *gb) = out
    lrel = float(((la - lb).abs() / lb.abs()).max())
    rels = [float((a.double() - b.double()).norm() / b.double().norm()) for a, b in zip(ga, gb)]
    coss = [float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0)) for a, b in zip(ga, gb)]
    print("activation decisions that differ between the two runs:", flips, "of", sum(a.size for a in decisions[0]),
          "| loss rel", lrel, "grad rel", rels, "1 - cos", [1 - c for c in coss])
    if dtype == "f32":
        assert lrel < 1e-6 and min(coss) > 1 - 1e-4, (lrel, rels, coss)
        assert max(rels) < (1e-5 if flips == 0 else 2e-2), (flips, rels)
    else:
        assert lrel < 2e-3 and min(coss) > 0.999, (lrel, coss)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paired_cycle_step_equals_one_network_at_a_time_with_the_option(sg, dtype):
    """The bounds of test_paired_cycle_step_is_bit_identical_to_one_network_at_a_time (d_quad off): losses, images and the table
    bitwise; parameter / slot / gradient buffers equal or within 1e-5 of their norm (shared weight-gradient launches)."""
    out, names = [], None
    for paired in (False, True):
        m = sg.sggan(sg.default_args(ngf=16, ndf=16, n_blocks=2, dtype=dtype, cycle=True, paired=paired, d_quad=False, diffaug="color,cutout"))
        m.real_A, m.seg_A, m.mask_A = _rand_inputs(2, 256, 256, m.discriminator, 61)
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(2, 256, 256, m.discriminator, 62)
        m.train_step()
        names = [f"net{k}.{what}" for k, n in enumerate(m.networks()) for what in ("flat", "m", "v", "grad")] + ["loss", "fake_A", "fake_B", "cyc_A", "cyc_B", "table"]
        out.append([t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.grad)] +
                   [m._loss.clone(), m.fake_A.tensor(), m.fake_B.tensor(), m.cyc_A.tensor(), m.cyc_B.tensor(), m.diffaug_params.clone()])
    for name, a, b in zip(names, *out):
        if torch.equal(a, b):
            continue
        assert name.startswith("net"), name
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        assert rel < 1e-5, (name, rel)


def test_checkpoint_resumes_to_the_bits_of_the_uninterrupted_run(sg):
    """The draws hang on the discriminators' step counters, which a checkpoint already carries: a model loaded from the state
    after step 2 reaches the bits of the uninterrupted step 4."""
    kw = dict(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=True, diffaug="color,cutout")
    a = sg.sggan(sg.default_args(**kw))
    sd = None
    for step in range(4):
        _feed(a, step)
        a.train_step()
        if step == 1:
            sd = {k: {kk: (vv.clone() if isinstance(vv, torch.Tensor) else vv) for kk, vv in v.items()} for k, v in a.state_dict().items()}
    b = sg.sggan(sg.default_args(**kw))
    b.load_state_dict(sd)
    for step in (2, 3):
        _feed(b, step)
        b.train_step()
    for x, y in zip(_state(a) + [a.diffaug_params], _state(b) + [b.diffaug_params]):
        assert torch.equal(x, y)


def test_data_parallel_rank_offsets_the_sample_index(sg):
    """Rank r of a data-parallel run holds samples r * N .. r * N + N - 1 of the concatenated batch and draws their rows: the
    table a model builds as rank 1 is the second half of the single-device table (the exchange itself is not needed for that)."""
    from types import SimpleNamespace
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", diffaug="color,cutout"))
    D = m.discriminator
    D.P.step_count = 3
    m._dp = SimpleNamespace(rank=1)
    got = m._diffaug_table(2, 64, 96, ((D, 0, 0), (D, 0, 1))).cpu().numpy()
    whole = [DO.param_rows(3, 19, 0, 4, role, 64, 96, 3) for role in (0, 1)]
    assert np.array_equal(got.view(np.uint32), np.concatenate([whole[0][2:], whole[1][2:]]).view(np.uint32))


def test_unet_cycle_step_runs_with_the_option(sg):
    m = sg.sggan(sg.default_args(ngf=8, ndf=8, dtype="bf16", cycle=True, use_resnet=False, diffaug="color,cutout"))
    _feed(m)
    m.train_step()
    gl, dl = m.losses()
    assert np.isfinite(gl) and np.isfinite(dl)
    assert all(bool(torch.isfinite(n.P.flat).all()) for n in m.networks())
    assert tuple(m.diffaug_params.shape) == (8, 8)


def test_option_with_the_image_pool_is_refused(sg):
    with pytest.raises(NotImplementedError, match="sample identity"):
        sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, cycle=True, use_pool=True, diffaug="color"))
    with pytest.raises(ValueError):
        sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, diffaug="translation"))
