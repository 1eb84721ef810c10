"""Training-mode dropout of the U-Net decoder on the MI355X path: sgg_dropout bit for bit against
tests/dropout_oracle.py at every block, chunk and grid-stride edge it has, under graph capture; a dropout unit, the generator
and its lockstep pair against float64; the model's steps (masks, bias gradient, graph replay, checkpoints, paired == unpaired,
inference callers untouched) and the option-off launch count."""
import numpy as np
import pytest
import torch

from tests import dropout_oracle as DO
from tests import unet_oracle as U
from tests.test_gpu_step import _l2, _rand_inputs, rel

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 16                      # elements in front of and behind the tensor (a multiple of 16 bytes in both dtypes)


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


@pytest.fixture(scope="module")
def K(sg):
    return sg.kernels


def _values(n, elems, dtype, seed=0):
    """Non-zero values the dtype holds, as float32 (n, elems): a zero in the result is a dropped element."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, elems)).astype(np.float32)
    x = np.where(np.abs(x) < 1e-3, np.float32(0.5), x)
    return torch.from_numpy(x).to(DT[dtype]).to(torch.float32).numpy()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _launch(K, x, dtype, rate, t, seed, stream_id, offset, it=None):
    """sgg_dropout on a guarded device copy of x (float32 values of the dtype): (result as a device tensor, guards untouched)."""
    n, elems = x.shape
    buf = torch.full((GUARD + n * elems + GUARD,), 7.0, dtype=DT[dtype], device="cuda")
    body = buf[GUARD:GUARD + n * elems].view(n, elems)
    body.copy_(torch.from_numpy(x))
    it = torch.tensor([t], dtype=torch.int64, device="cuda") if it is None else it
    K.dropout_(body, rate, it, seed, offset, stream_id)
    torch.cuda.synchronize()
    return body, bool((buf[:GUARD] == 7.0).all() and (buf[GUARD + n * elems:] == 7.0).all())


def _expect(x, dtype, rate, t, seed, stream_id, offset):
    n, elems = x.shape
    keep = DO.keep_mask(t, seed, stream_id, offset, n, elems, rate)
    return torch.from_numpy(DO.apply(x, keep, rate, bf16=dtype == "bf16")).to(DT[dtype]), keep


def _check(K, n, elems, dtype, rate=0.5, t=1, seed=19, stream_id=0, offset=0):
    x = _values(n, elems, dtype, seed=elems % 1000 + n)
    got, guards = _launch(K, x, dtype, rate, t, seed, stream_id, offset)
    want, keep = _expect(x, dtype, rate, t, seed, stream_id, offset)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"({n}, {elems}) {dtype} rate {rate} t {t} stream {stream_id}: {int(bad.sum())} elements differ, first at {np.argwhere(bad)[0].tolist()}"
    assert guards, "guard cells around the buffer were written"
    return x, got, keep


def _edge_sizes(K):
    """(n, elems): the issue's list, then one vector count on either side of every boundary of csrc/dropout.hip -- the thread
    stride DROPOUT_THREADS (255 / 256 / 257 vectors, in the list), the chunk DROPOUT_CHUNK, and the grid stride: with n samples
    a block row holds DROPOUT_GRID_BLOCKS / n blocks, so a sample of more than that many chunks sends its blocks round again."""
    T, CH, GB = K.DROPOUT_THREADS, K.DROPOUT_CHUNK, K.DROPOUT_GRID_BLOCKS
    assert (T, CH, GB) == (256, 1024, 2048)
    base = [(1, 8), (2, 8 * (T - 1)), (2, 8 * T), (2, 8 * (T + 1)), (3, 16 * 16 * 64)]
    chunk = [(2, 8 * (CH - 1)), (2, 8 * CH), (2, 8 * (CH + 1))]
    wrap = [(2, 8 * (GB // 2 * CH)), (2, 8 * (GB // 2 * CH + 1)), (GB, 8 * (CH + 1)), (GB + 1, 8 * (CH + 1))]    # (n >= GB: one block per sample)
    return base + chunk + wrap


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_kernel_matches_the_oracle_bit_for_bit_at_every_edge(K, dtype):
    for n, elems in _edge_sizes(K):
        if n >= K.DROPOUT_GRID_BLOCKS:           # (many short samples, each with a mask of its own: four rows are compared)
            x = _values(n, elems, dtype, seed=n)
            got, guards = _launch(K, x, dtype, 0.5, 1, 19, 0, 0)
            for r in (0, 1, n // 2, n - 1):
                want, _ = _expect(x[r:r + 1], dtype, 0.5, 1, 19, 0, r)
                assert np.array_equal(_bits(got[r:r + 1]), _bits(want)), (n, elems, r)
            assert guards
        else:
            _check(K, n, elems, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_kernel_rates_counters_streams_and_offsets(K, dtype):
    n, elems = 3, 16 * 16 * 64
    for rate in (0.0, 0.2, 0.5):
        for t in (0, 1, 2 ** 32 + 5):
            for stream_id in (0, 5):
                x, got, keep = _check(K, n, elems, dtype, rate=rate, t=t, stream_id=stream_id)
                if rate == 0.0:
                    assert keep.all() and np.array_equal(_bits(got), _bits(torch.from_numpy(x).to(DT[dtype])))     # every bit of x
                else:
                    assert np.array_equal(got.float().cpu().numpy() != 0, keep)
    # sample_offset 5 reproduces rows 5.. of an offset-0 launch
    x = _values(8, elems, dtype, seed=3)
    full, _ = _launch(K, x, dtype, 0.5, 7, 21, 2, 0)
    tail, _ = _launch(K, x[5:], dtype, 0.5, 7, 21, 2, 5)
    assert torch.equal(full[5:], tail) and not torch.equal(full[:3], tail)
    # a second call on a fresh copy gives the same bits
    again, _ = _launch(K, x, dtype, 0.5, 7, 21, 2, 0)
    assert torch.equal(full, again)


def test_f32_and_bf16_drop_the_same_elements(K):
    n, elems = 3, 8 * 1025
    x = _values(n, elems, "bf16", seed=9)
    a, _ = _launch(K, x, "f32", 0.2, 3, 19, 1, 0)
    b, _ = _launch(K, x, "bf16", 0.2, 3, 19, 1, 0)
    keep = DO.keep_mask(3, 19, 1, 0, n, elems, 0.2)
    assert np.array_equal(a.cpu().numpy() != 0, keep) and np.array_equal(b.float().cpu().numpy() != 0, keep)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_kernel_under_graph_capture_reads_the_counter_when_it_runs(K, dtype):
    n, elems = 2, 8 * 1025
    x = _values(n, elems, dtype, seed=5)
    src = torch.from_numpy(x).to("cuda").to(DT[dtype])
    buf = src.clone()
    it = torch.tensor([3], dtype=torch.int64, device="cuda")
    K.dropout_(buf, 0.5, it, 19, 0, 1)                                   # warm-up (module load) outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.dropout_(buf, 0.5, it, 19, 0, 1)
    for t in (3, 2 ** 32 + 9):
        buf.copy_(src)
        it.fill_(t)
        graph.replay()
        torch.cuda.synchronize()
        want, _ = _expect(x, dtype, 0.5, t, 19, 1, 0)
        assert np.array_equal(_bits(buf), _bits(want)), t


# ----------------------------------------------------------------------------- unit level
def _t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _nchw(a):
    return _t64(a).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def _close(got, exp, what, bar=2e-4, entry=1e-3):
    a, b = _l2(got, exp), rel(got, exp)
    print(f"{what}: relative L2 {a:.2e}, worst entry / largest {b:.2e}")
    assert a < bar and b < entry, (what, a, b)


@pytest.mark.parametrize("name", ["d1", "d3"])
def test_dropout_unit_forward_backward_against_float64(sg, name):
    """A d1-type unit (deconv -> mask -> IN -> + skip) and the d3-type unit with skip_grad (... -> ReLU), f32, N 2, 16x16, 64 -> 64
    channels, forward and backward with dropout against float64: y, dx, dW, db (non-zero), dgamma, dbeta and the skip gradient.
    The ReLU of the d3 form takes its decisions from the kernel's own output.  Bars of tests/test_gpu_unet.py: image 1e-4,
    gradients relative L2 2e-4, single entries 1e-3 of the tensor's largest."""
    G = sg.GeneratorUNet(gf_dim=8, dtype=torch.float32, seed=23)
    u = getattr(G, "dec")[int(name[1]) - 1]
    assert u.drop_layer == int(name[1]) - 1 and (u.cin, u.cout) == (64, 64) and u.skip_grad == (name == "d3")
    rng = np.random.default_rng(31)
    P = {k: v.astype(np.float64) for k, v in G.P.export().items()}
    for k in (name + "_b", name + "_g", name + "_beta"):
        P[k] = (P[k] + 0.2 * rng.standard_normal(P[k].shape)).astype(np.float32).astype(np.float64)
    G.P.load(P)
    G.P.step_count = 3
    N, H, W, C = 2, 16, 16, 64
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    x, skip, dy = f32(rng.standard_normal((N, H, W, C))), f32(rng.standard_normal((N, H, W, C))), f32(rng.standard_normal((N, H, W, C)))
    dev = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")
    drop = (4 * 1 + u.drop_layer, 6)                                      # application 1, sample offset 6
    G.P.zero_grad()
    y, rec = u.forward(dev(x), residual=dev(skip), drop=drop)
    assert rec[-1] == drop
    keep = DO.layer_mask(3, 23, drop[0], 6, N, H, W, C, 0.5)
    assert np.array_equal(rec[2].cpu().numpy() != 0, keep)                # the recorded pre-norm tensor is the masked one
    out = u.backward(rec, dev(dy), True, True)
    dx, dskip = out if u.skip_grad else (out, None)
    # float64
    tx, tskip = _nchw(x).requires_grad_(True), _nchw(skip).requires_grad_(True)
    tp = {k: _t64(P[name + k]).requires_grad_(True) for k in ("_w", "_b", "_g", "_beta")}
    pre = DO.masked_deconv_norm(tx, tp["_w"], tp["_b"], tp["_g"], tp["_beta"], _nchw(keep.astype(np.float64)), 2.0) + tskip
    ye = pre * _nchw((y > 0).cpu().numpy().astype(np.float64)) if u.skip_grad else pre
    (ye * _nchw(dy)).sum().backward()
    if u.skip_grad:                                                        # the kernel's branch is the oracle's outside the rounding band
        assert not ((y > 0).cpu().numpy() != (_nhwc(pre) > 0))[np.abs(_nhwc(pre)) > 1e-4].any()
    assert rel(y.cpu().numpy(), _nhwc(ye)) < 1e-4
    got = G.P.export(G.P.grad)
    _close(dx.cpu().numpy(), _nhwc(tx.grad), name + " dx")
    for k in ("_w", "_b", "_g", "_beta"):
        _close(got[name + k], tp[k].grad.numpy(), name + " d" + k[1:])
    assert np.abs(got[name + "_b"]).min() > 0
    if u.skip_grad:
        _close(dskip.cpu().numpy(), _nhwc(tskip.grad), name + " dskip")
    # inference mode on the same unit: the bias gradient stays exactly 0
    G.P.zero_grad()
    y0, rec0 = u.forward(dev(x), residual=dev(skip))
    u.backward(rec0, dev(dy), True, True)
    assert len(rec0) == len(rec) - 1 and float(G.P.g(name + "_b").abs().max()) == 0.0


# ----------------------------------------------------------------------------- generator level
def _generator_case(sg, seed=19):
    G = sg.GeneratorUNet(gf_dim=8, dtype=torch.float32, seed=seed)
    rng = np.random.default_rng(40 + seed)
    P = {k: v.astype(np.float64) for k, v in G.P.export().items()}
    for k in P:
        if not k.endswith("_w"):
            P[k] = (P[k] + 0.1 * rng.standard_normal(P[k].shape)).astype(np.float32).astype(np.float64)
    G.P.load(P)
    G.P.step_count = 2
    x = rng.uniform(0, 1, (2, 16, 16, 3)).astype(np.float32)
    dy = rng.standard_normal((2, 16, 16, 3)).astype(np.float32)
    return G, P, x, dy


def test_generator_forward_backward_with_dropout_against_the_masked_oracle(sg, K):
    """GeneratorUNet(gf_dim=8), N 2, 16x16, f32: forward(x, dropout=0) and backward against tests/dropout_oracle's masked float64
    statement, kink-aware as tests/test_gpu_unet.py is (the oracle's own decisions except within 1e-4 of a kink, where the
    kernel's recorded ones are taken; none may differ outside).  Then generator(x, training=True) through torch autograd: the
    same gradients, bit for bit."""
    G, P, x, dy = _generator_case(sg)
    xi = G.to_internal(torch.from_numpy(x).cuda())
    dyi = K.pad_channels(torch.from_numpy(dy).cuda(), 8, torch.float32)
    G.P.zero_grad()
    y, tape = G.forward(xi, dropout=0)
    dx = G.backward(tape, dyi, want_dx=True)
    grads = G.P.export(G.P.grad)
    flat = G.P.grad.clone()
    masks = DO.nchw_masks(2, 19, 0, 0, 2, 16, 16, 64, 0.5)
    for l in range(3):
        assert np.array_equal(tape[8 + l][2].cpu().numpy() != 0, _nhwc(masks[l]) != 0), f"d{l + 1}: recorded pre-norm tensor"
    kinks = DO.Kinks([torch.from_numpy(b).permute(0, 3, 1, 2) for b in U.unet_branches(G, tape)])
    tp = {k: _t64(v).requires_grad_(True) for k, v in P.items()}
    tx = _nchw(x.astype(np.float64)).requires_grad_(True)
    ye = DO.torch_generator_unet(tp, tx, masks, 0.5, kinks=kinks)
    (ye * _nchw(dy.astype(np.float64))).sum().backward()
    print(f"kink-aware masked oracle: {kinks.ambiguous} decisions within 1e-4, {kinks.disagree_outside} differ outside")
    assert kinks.calls == 10 and kinks.disagree_outside == 0
    assert rel(y[..., :3].cpu().numpy(), _nhwc(ye)) < 1e-4
    _close(dx[..., :3].cpu().numpy(), _nhwc(tx.grad), "dx")
    for k, v in grads.items():
        if k.endswith("_b") and k not in ("d1_b", "d2_b", "d3_b", "d8_b"):   # a bias in front of an unmasked norm: exactly 0
            assert np.abs(v).max() == 0.0 and np.abs(tp[k].grad.numpy()).max() < 1e-9, k
            continue
        _close(v, tp[k].grad.numpy(), k)
    assert all(np.abs(grads[k]).min() > 0 for k in ("d1_b", "d2_b", "d3_b"))
    # Keras's keyword through the autograd facade: application 0, sample offset 0
    G.requires_grad_(True)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    out = G(xt, training=True)
    assert torch.equal(out, K.unpad_channels(y, 3))
    out.backward(torch.from_numpy(dy).cuda())
    assert torch.equal(xt.grad, K.unpad_channels(dx, 3))
    for n, v in zip(G.P.names(), G.trainable_variables):
        assert torch.equal(v.grad, G.P.g(n, buf=flat)), n
    G.requires_grad_(False)
    assert not torch.equal(G(torch.from_numpy(x).cuda()), out.detach())    # the default is inference mode ...
    assert torch.equal(G(torch.from_numpy(x).cuda()), G(torch.from_numpy(x).cuda(), training=False))
    R = sg.Generator(gf_dim=8, n_blocks=1, dtype=torch.float32)            # ... and the ResNet accepts the keyword and ignores it
    xr = torch.rand(1, 32, 32, 3, device="cuda")
    assert torch.equal(R(xr, training=True), R(xr))


def test_generator_pair_with_dropout_equals_one_network_at_a_time(sg):
    """GeneratorUNetPair masks each half with its own network's seed and counter: outputs, data gradients and every parameter
    gradient equal the two networks run one at a time, bit for bit."""
    from sggan_amd.module import GeneratorUNetPair
    Ga, _, x, dy = _generator_case(sg, 19)
    Gb, _, _, _ = _generator_case(sg, 21)
    Gb.P.step_count = 5
    rng = np.random.default_rng(77)
    xs = Ga.to_internal(torch.from_numpy(rng.uniform(0, 1, (4, 16, 16, 3)).astype(np.float32)).cuda())
    dys = Ga.to_internal(torch.from_numpy(rng.standard_normal((4, 16, 16, 3)).astype(np.float32)).cuda())
    pair = GeneratorUNetPair(Ga, Gb)
    Ga.P.zero_grad(); Gb.P.zero_grad()
    yp, tp = pair.forward(xs, dropout=1, sample_offset=3)
    dxp = pair.backward(tp, dys, want_dx=True)
    gp = (Ga.P.grad.clone(), Gb.P.grad.clone())
    for l in range(3):
        for h, (G, t) in enumerate(((Ga, 2), (Gb, 5))):
            keep = DO.layer_mask(t, G.seed, 4 + l, 3, 2, 16, 16, 64, 0.5)
            assert np.array_equal(tp[8 + l][2][2 * h:2 * h + 2].cpu().numpy() != 0, keep), (l, h)
    for h, G in enumerate((Ga, Gb)):
        sl = slice(2 * h, 2 * h + 2)
        G.P.zero_grad()
        y, t = G.forward(xs[sl].contiguous(), dropout=1, sample_offset=3)
        dx = G.backward(t, dys[sl].contiguous(), want_dx=True)
        assert torch.equal(y, yp[sl]) and torch.equal(dx, dxp[sl]), h
        for n in G.P.names():
            assert torch.equal(G.P.g(n), G.P.g(n, buf=gp[h])), (h, n)


# ----------------------------------------------------------------------------- model level
KW = dict(use_resnet=False, ngf=8, ndf=8)


def _feed(m, step=0, N=2):
    m.real_A, m.seg_A, m.mask_A = _rand_inputs(N, 128, 128, m.discriminator, 60 + step)
    if m.cycle:
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(N, 128, 128, m.discriminator, 80 + step)


def _zero_pattern_is_mask(xc, t, seed, stream_id, what):
    n, H, W, C = xc.shape
    keep = DO.layer_mask(t, seed, stream_id, 0, n, H, W, C, 0.5)
    assert np.array_equal(xc.float().cpu().numpy() != 0, keep), what


def test_reference_step_masks_and_bias_gradient(sg):
    """After a step with keep_tapes the zero pattern of each recorded pre-norm tensor of d1..d3 equals keep_mask at the counter
    value BEFORE the update (the second step: t = 1), stream 4 * 0 + layer, sample offset 0; d1_b's gradient is non-zero with the
    option and exactly 0 without it."""
    m = sg.sggan(sg.default_args(dtype="f32", keep_tapes=True, dropout=0.5, **KW))
    assert m.dropout == 0.5 and m.generator.dropout == 0.5
    for step in range(2):
        _feed(m, step)
        m.train_step()
    assert m.generator.P.step_count == 2
    for l in range(3):
        _zero_pattern_is_mask(m.tapes["G"][8 + l][2], 1, m.generator.seed, l, f"d{l + 1}")
    g = m.generator.P.export(m.generator.P.grad)
    assert all(np.abs(g[k]).max() > 0 for k in ("d1_b", "d2_b", "d3_b")) and np.abs(g["d4_b"]).max() == 0.0
    off = sg.sggan(sg.default_args(dtype="f32", **KW))
    _feed(off)
    off.train_step()
    g0 = off.generator.P.export(off.generator.P.grad)
    assert all(np.abs(g0[k]).max() == 0.0 for k in ("d1_b", "d2_b", "d3_b"))


def test_cycle_step_masks_of_both_applications_of_both_generators(sg):
    m = sg.sggan(sg.default_args(dtype="f32", keep_tapes=True, dropout=0.5, cycle=True, paired=True, **KW))
    for step in range(2):
        _feed(m, step)
        m.train_step()
    n = 2
    Gab, Gba = m.generator, m.generator_BA
    assert (Gab.seed, Gba.seed) == (19, 21)
    # G_first = (G_AB; G_BA) over the real batches: application 0; G_second = (G_BA; G_AB) over the fakes: application 1
    for key, app, nets in (("G_first", 0, (Gab, Gba)), ("G_second", 1, (Gba, Gab))):
        for l in range(3):
            xc = m.tapes[key][8 + l][2]
            for h, G in enumerate(nets):
                _zero_pattern_is_mask(xc[h * n:(h + 1) * n], 1, G.seed, 4 * app + l, (key, l, h))
    for G in (Gab, Gba):
        g = G.P.export(G.P.grad)
        assert all(np.abs(g[k]).max() > 0 for k in ("d1_b", "d2_b", "d3_b"))


def _run_steps(sg, steps, **kw):
    m = sg.sggan(sg.default_args(**{**KW, "dropout": 0.5, **kw}))
    out = []
    for step in range(steps):
        _feed(m, step)
        m.train_step()
        out.append([t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.iterations, n.P.grad)]
                   + [m._loss.clone(), m.fake_A.tensor().clone()])
    return m, out


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_replay_equals_eager_bitwise(sg, dtype, cycle):
    _, eager = _run_steps(sg, 3, dtype=dtype, cycle=cycle, graph=False)
    mg, graph = _run_steps(sg, 3, dtype=dtype, cycle=cycle, graph=True)
    assert mg._program is not None
    for step, (a, b) in enumerate(zip(eager, graph)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (step, i)
    assert all(torch.isfinite(t.float()).all() for t in graph[-1])         # (bf16: losses and gradients are finite)
    assert not torch.equal(eager[0][-1], _run_steps(sg, 1, dtype=dtype, cycle=cycle, dropout=None)[1][0][-1])     # the option does something


def test_one_step_save_load_one_step_equals_two_steps(sg):
    _, two = _run_steps(sg, 2, dtype="f32")
    m1, _ = _run_steps(sg, 1, dtype="f32")
    sd = m1.state_dict()
    m2 = sg.sggan(sg.default_args(dropout=0.5, dtype="f32", **KW))
    m2.load_state_dict(sd)
    _feed(m2, 1)
    m2.train_step()
    got = [t for n in m2.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.iterations, n.P.grad)] + [m2._loss, m2.fake_A.tensor()]
    for i, (a, b) in enumerate(zip(two[1], got)):
        assert torch.equal(a, b), i


def test_paired_and_unpaired_cycle_steps_agree_bitwise(sg):
    out = []
    for paired in (False, True):
        m = sg.sggan(sg.default_args(dropout=0.5, dtype="f32", cycle=True, paired=paired, d_quad=False, **KW))
        _feed(m)
        m.train_step()
        assert (getattr(m, "_pairs", None) is not None) == paired
        out.append([t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.grad)]
                   + [m._loss.clone(), m.fake_A.tensor(), m.fake_B.tensor(), m.cyc_A.tensor(), m.cyc_B.tensor()])
    for i, (a, b) in enumerate(zip(*out)):
        assert torch.equal(a, b), i


def test_inference_callers_are_untouched_by_the_option(sg, tmp_path):
    """generator(x) and the epoch-end test pass of a model built with the option give the bits of an option-off model holding
    the same weights."""
    from sggan_amd.main import parse_args, synthetic_test_samples
    argv = ["--generator", "unet", "--img_height", "128", "--img_width", "128", "--ngf", "8", "--ndf", "8", "--dtype", "f32",
            "--batch_size", "2", "--test_dir", str(tmp_path / "t")]
    a_on, a_off = parse_args(argv + ["--dropout"]), parse_args(argv)
    assert a_on.dropout == 0.5 and not hasattr(a_off, "dropout")
    on, off = sg.sggan(a_on), sg.sggan(a_off)
    _feed(on)
    on.train_step()
    for p, q in zip(on.networks(), off.networks()):
        q.P.flat.copy_(p.P.flat); q.P.version += 1
    x = torch.rand(2, 128, 128, 3, device="cuda")
    assert torch.equal(on.generator(x), off.generator(x))
    samples = synthetic_test_samples(a_on, count=2)
    f_on, s_on = on.test_during_train(0, a_on, samples(0), None)
    f_off, s_off = off.test_during_train(0, a_off, samples(0), None)
    assert np.array_equal(f_on, f_off)
    np.testing.assert_equal(s_on, s_off)                                   # (the scores of the same images; a class nobody has is NaN in both)


# launches of the U-Net reference step at 2 x 128 x 128, bf16, ngf = ndf = 8, counted with tests/test_gpu_spectral._captured_nodes
# on the parent commit (ffd3859, the same procedure on a checkout of it)
PARENT_UNET_REFERENCE_NODES = 249


def test_option_off_launch_count_and_state_dict_keys(sg):
    from tests.test_gpu_spectral import _captured_nodes
    m = sg.sggan(sg.default_args(dtype="bf16", **KW))
    assert m.dropout is None
    sd = m.state_dict()
    assert set(sd) == {"G", "D"} and set(sd["G"]) == {"flat", "m", "v", "t", "arch"} and set(sd["D"]) == {"flat", "m", "v", "t"}
    on = sg.sggan(sg.default_args(dtype="bf16", dropout=0.5, **KW))
    assert {k: set(v) for k, v in on.state_dict().items()} == {k: set(v) for k, v in sd.items()}        # the option adds no state
    counts = {}
    for name, model in (("off", m), ("on", on)):
        _feed(model)
        model.train_step()
        model._stage_inputs()
        torch.cuda.synchronize()
        counts[name] = _captured_nodes(model.device, model._step_body)
    print("captured nodes of the U-Net reference step:", counts)
    assert counts["off"] == PARENT_UNET_REFERENCE_NODES
    assert counts["on"] == counts["off"] + 3 * 4            # per site: the forward mask, the backward mask, the bias gradient's two
