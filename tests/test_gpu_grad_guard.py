"""GPU tests of the guarded optimizer step (sgg_grad_sumsq / sgg_adam_guard, --clip_grad_norm / --skip_nonfinite).

The reference for the update is the existing entry point: sgg_adam_iter (sgg_adam_sched with a schedule) called with the
gradient factor the guard decided -- the same device arithmetic on the same f32 values, so those comparisons are BITWISE.
The reference for the norm is the correctly rounded float64 sum of the exact squares (math.fsum).  Sizes sit at the edges of
the sum-of-squares pass (CHUNK elements per block, 16-byte groups, a scalar tail), not at the networks' own sizes."""
import functools
import math
import os
import warnings

import numpy as np
import pytest
import torch

from tests.test_gpu_step import _rand_inputs

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-7
CHUNK = 8192
# tail only / one group / group + tail / a part chunk / one whole chunk / one element into the second / three chunks with a
# 3-element tail / 258 chunks: the fold of the chunk records takes a second round (256 threads, records k and k + 256)
SIZES = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, 257 * CHUNK + 5]
U64 = float(np.finfo(np.float64).eps)          # ulp(f64) at 1 = 2^-52


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    import sggan_amd.kernels, sggan_amd.main  # noqa: F401,E401
    assert sggan_amd.kernels.GRAD_GUARD_CHUNK == CHUNK
    return sggan_amd


@functools.lru_cache(maxsize=None)
def _problem(n):
    """theta0 and three gradients (host f32 tensors; generated once per size, never written)."""
    g = torch.Generator().manual_seed(2000 + n % 997)
    return torch.randn(n, generator=g), tuple(torch.randn(n, generator=g) * 0.1 for _ in range(3))


@functools.lru_cache(maxsize=None)
def _norm64(n, k=0):
    """The oracle: sqrt of the correctly rounded sum of the squares, which are exact in float64."""
    return math.sqrt(math.fsum((_problem(n)[1][k].double() ** 2).tolist()))


class _Slots:
    def __init__(self, sg, theta):
        n = theta.numel()
        self.K = sg.kernels
        self.theta, self.m, self.v = theta.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        self.state = torch.zeros(2, dtype=torch.int64, device="cuda")
        self.guard = torch.zeros(4, dtype=torch.float64, device="cuda")
        self.ws = self.K.grad_guard_workspace(n, "cuda")

    def guarded(self, g, sched=None, grad_scale=1.0, max_norm=0.0):
        self.K.adam_guard(self.theta, g, self.m, self.v, self.state, self.guard, self.ws, sched, LR, B1, B2, EPS, grad_scale, max_norm)

    def plain(self, g, sched=None, grad_scale=1.0):
        if sched is None:
            self.K.adam_iter(self.theta, g, self.m, self.v, self.state, LR, B1, B2, EPS, grad_scale)
        else:
            self.K.adam_sched(self.theta, g, self.m, self.v, self.state, sched, LR, B1, B2, EPS, grad_scale)

    def bits(self):
        return [self.theta.view(torch.int32).clone(), self.m.view(torch.int32).clone(), self.v.view(torch.int32).clone(),
                self.state[0:1].clone()]


def _same(a, b, what):
    for name, x, y in zip(("theta", "m", "v", "iterations"), a, b):
        assert torch.equal(x, y), (what, name)


@pytest.mark.parametrize("n", SIZES)
def test_norm_against_the_float64_oracle_and_twice_the_same_bits(sg, n):
    """last_norm within 4 ulp(f64) * sqrt(n), relative, of the oracle -- the bound the feature was specified with.  That the
    kernels must meet it follows from their summation depth, not from a measurement: every term x^2 is exact and non-negative,
    so the computed sum is sum x_i^2 (1 + d_i) with |d_i| <= D u, u = 2^-53, D the number of additions a term passes through:
    at most 32 in its thread (8 groups of 4), 8 in the block's tree, ceil(chunks / 256) in the fold and 8 in its tree --
    D <= 48 + ceil(n / 2^21), and never more than n - 1, since adding zero is exact.  The square root halves the relative
    error and rounds once, the product with grad_scale rounds once: |norm - oracle| / oracle <= (min(n - 1, D) / 2 + 2) u (the
    oracle adds at most 1 u of its own), which is below 8 u sqrt(n) = 4 ulp sqrt(n) for every n >= 1.
    Two runs -- other buffers, other workspace -- give the same bits in every chunk record and in the norm."""
    K = sg.kernels
    theta0, grads = _problem(n)
    g = grads[0].cuda()
    chunks = -(-n // CHUNK)
    runs = []
    for _ in range(2):
        s = _Slots(sg, theta0)
        sums, flags = K.grad_sumsq(g, s.ws)
        assert sums.numel() == flags.numel() == chunks and int(flags.abs().sum().item()) == 0
        part = sums.clone()
        s.guarded(g)
        rec = s.guard.cpu()
        assert torch.equal(s.ws[16:16 + 16 * chunks].view(torch.float64)[0::2], part)      # the call ran the same partial pass
        runs.append((part.view(torch.int64), rec.view(torch.int64)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    norm, clip, skipped, applied = rec.tolist()
    oracle = _norm64(n)
    depth = min(n - 1, 48 + -(-n // (1 << 21)))
    err = abs(norm - oracle) / oracle
    print(f"n = {n}: |norm - oracle| / oracle = {err:.3e} = {err / U64:.2f} ulp; derived bound {(depth / 2 + 3) / 2:.1f} ulp; "
          f"required {4 * math.sqrt(n):.1f} ulp")
    assert err <= (depth / 2 + 3) * (U64 / 2) <= 4 * U64 * math.sqrt(n)
    assert err <= 4 * U64 * math.sqrt(n)
    assert (clip, skipped, applied) == (1.0, 0.0, 1.0)
    first = math.fsum((grads[0][:CHUNK].double() ** 2).tolist())                           # and the first chunk's own record
    assert abs(part[0].item() - first) <= 41 * (U64 / 2) * first


@pytest.mark.parametrize("n", SIZES)
def test_guard_off_is_bitwise_the_plain_update(sg, n):
    """max_norm = 0 and finite gradients: theta, m, v and iterations after each of three steps equal sgg_adam_iter's and, with a
    schedule whose third step decays, sgg_adam_sched's -- bit for bit; so does a clip bound the norm stays under."""
    theta0, grads = _problem(n)
    for sched_host in (None, (1, 1, 4)):
        sched = None if sched_host is None else torch.tensor(sched_host, dtype=torch.int64, device="cuda")
        a, b, c = _Slots(sg, theta0), _Slots(sg, theta0), _Slots(sg, theta0)
        for it in range(3):
            g = grads[it].cuda()
            a.guarded(g, sched)
            b.plain(g, sched)
            c.guarded(g, sched, max_norm=2.0 * _norm64(n, it))
            _same(a.bits(), b.bits(), (n, sched_host, it))
            _same(c.bits(), b.bits(), (n, sched_host, it, "under the bound"))
        assert a.state[0].item() == 3 and a.guard.tolist()[1:] == [1.0, 0.0, 3.0] and c.guard.tolist()[1:] == [1.0, 0.0, 3.0]
    if n > 1:
        d = _Slots(sg, theta0)
        d.plain(grads[0].cuda())
        assert not torch.equal(d.theta.cpu(), theta0)                                      # (the steps did move something)


@pytest.mark.parametrize("n", SIZES)
def test_clip_is_bitwise_the_plain_update_at_the_clipped_scale(sg, n):
    """max_norm = half the measured norm (grad_scale 1, then 1/2 as a two-rank run would pass): the record's clip is the oracle's
    f32 value, float32(max_norm / norm) from the record's own norm, and the update equals sgg_adam_iter called with
    grad_scale * clip formed in f32."""
    K = sg.kernels
    theta0, grads = _problem(n)
    f = np.float32
    for gs in (1.0, 0.5):
        a, b = _Slots(sg, theta0), _Slots(sg, theta0)
        for it in range(2):
            g = grads[it].cuda()
            max_norm = float(f(0.5 * gs * _norm64(n, it)))
            a.guarded(g, grad_scale=gs, max_norm=max_norm)
            norm, clip = a.guard.tolist()[:2]
            assert abs(norm - gs * _norm64(n, it)) <= 4 * U64 * math.sqrt(n) * norm
            assert clip == float(f(max_norm / norm)) and abs(clip - 0.5) < 1e-6
            info = K.guarded_update(theta0.numpy(), grads[it].numpy(), 0 * theta0.numpy(), 0 * theta0.numpy(), it, LR, B1, B2, EPS, gs, max_norm)[4]
            assert clip == info["clip"] and not info["skip"]
            b.plain(g, grad_scale=float(f(gs) * f(clip)))
            _same(a.bits(), b.bits(), (n, gs, it))
        assert a.guard.tolist()[2:] == [0.0, 2.0]


def _positions(n):
    """first / last element, both sides of each chunk boundary, the first element of the scalar tail and the one before it."""
    p = {0, n - 1, n - n % 4, n - n % 4 - 1, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, 256 * CHUNK}
    return sorted(i for i in p if 0 <= i < n)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "neg_inf"])
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_gradient_is_skipped_and_the_next_step_applies(sg, n, bad):
    """After one applied step, a gradient with ONE non-finite element -- at each edge position in turn -- leaves theta, m, v and
    iterations with every bit, writes the scratch rate as 0, counts one skip and flags exactly the chunk that holds the element;
    the finite step after all of them applies with t = iterations + 1 = 2, bitwise as two plain steps.  With and without a
    clip bound (clipping implies the skip)."""
    K = sg.kernels
    theta0, grads = _problem(n)
    a, b = _Slots(sg, theta0), _Slots(sg, theta0)
    a.guarded(grads[0].cuda()); b.plain(grads[0].cuda())
    before = a.bits()
    g = grads[1].clone().cuda()
    skipped = 0
    for pos in _positions(n):
        for max_norm in (0.0, 1e-3):
            keep = g[pos].item()
            g[pos] = bad
            a.guarded(g, max_norm=max_norm)
            skipped += 1
            _same(a.bits(), before, (n, pos, max_norm))
            norm, clip, sk, ap = a.guard.tolist()
            assert not math.isfinite(norm) and clip == 1.0 and (sk, ap) == (float(skipped), 1.0), (n, pos, a.guard.tolist())
            assert a.state[1:].view(torch.float32)[0].item() == 0.0 and a.ws[:4].view(torch.int32).item() == 1
            flags = a.ws[16:16 + 16 * (-(-n // CHUNK))].view(torch.int32)[2::4]
            assert flags.nonzero().flatten().tolist() == [pos // CHUNK], (n, pos)
            g[pos] = keep
    a.guarded(grads[2].cuda()); b.plain(grads[2].cuda())
    _same(a.bits(), b.bits(), (n, "the step after the skips"))
    assert a.state[0].item() == 2 and a.guard.tolist()[1:] == [1.0, float(skipped), 2.0]


def test_finite_gradient_whose_f32_sum_of_squares_overflows_is_clipped_not_skipped(sg):
    """Values near 1e20: every element is finite, the sum of squares (1e40 per element) is past f32 but not past the double
    the pass accumulates in -- the step is clipped to max_norm = 1 and applied, bitwise as sgg_adam_iter at that factor."""
    n = 2 * CHUNK + 7
    theta0, grads = _problem(n)
    f = np.float32
    big = grads[0] * 1e21
    assert torch.isfinite(big).all() and torch.isinf((big * big).sum())
    a, b = _Slots(sg, theta0), _Slots(sg, theta0)
    a.guarded(big.cuda(), max_norm=1.0)
    norm, clip, sk, ap = a.guard.tolist()
    oracle = math.sqrt(math.fsum((big.double() ** 2).tolist()))
    assert (sk, ap) == (0.0, 1.0) and abs(norm - oracle) <= 4 * U64 * math.sqrt(n) * oracle and norm > 1e20
    assert clip == float(f(1.0 / norm)) and 0.0 < clip < 1e-20
    b.plain(big.cuda(), grad_scale=float(f(1.0) * f(clip)))
    _same(a.bits(), b.bits(), "overflow")
    assert torch.isfinite(a.theta).all() and not torch.equal(a.theta.cpu(), theta0)


def test_guarded_update_statement_tracks_the_kernel(sg):
    """kernels.guarded_update (float64) against the device over a clipped, a skipped and a plain step with a schedule: the same
    decisions, theta / m / v at the bound tests/test_gpu_ops.py holds sgg_adam to against its float64 oracle (2e-6)."""
    K = sg.kernels
    n = CHUNK + 1
    theta0, grads = _problem(n)
    sched_host = (1, 1, 4)
    sched = torch.tensor(sched_host, dtype=torch.int64, device="cuda")
    a = _Slots(sg, theta0)
    th, m, v, it = theta0.double().numpy(), np.zeros(n), np.zeros(n), 0
    nan_g = grads[1].clone(); nan_g[n - 1] = float("nan")
    for g, max_norm in ((grads[0], 0.5), (nan_g, 0.5), (grads[2], 0.0)):
        a.guarded(g.cuda(), sched, max_norm=max_norm)
        th, m, v, it, info = K.guarded_update(th, g.numpy(), m, v, it, LR, B1, B2, EPS, 1.0, max_norm, sched_host)
        norm, clip = a.guard.tolist()[:2]
        assert clip == info["clip"] and a.state[0].item() == it
        assert info["skip"] or abs(norm - info["norm"]) <= 1e-12 * norm
    assert it == 2 and a.guard.tolist()[2:] == [1.0, 2.0]
    for x, y in ((a.theta, th), (a.m, m), (a.v, v)):
        assert np.abs(x.cpu().numpy() - y).max() < 2e-6


def test_guarded_update_replays_from_a_captured_graph(sg):
    """One adam_guard call captured; the replays decide from device memory: a plain gradient, a NaN, a large gradient (clipped)
    -- equal to the same three eager calls bitwise, record included."""
    n = 2 * CHUNK + 7
    theta0, grads = _problem(n)
    seq = [grads[0], grads[1].clone(), grads[2] * 1e3]
    seq[1][CHUNK] = float("nan")
    max_norm = 2.0 * _norm64(n)
    e = _Slots(sg, theta0)
    for g in seq:
        e.guarded(g.cuda(), max_norm=max_norm)
    c = _Slots(sg, theta0)
    g_static = torch.zeros(n, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.guarded(g_static, max_norm=max_norm)
    assert c.state[0].item() == 0 and c.guard.tolist() == [0.0] * 4                        # capturing ran nothing
    for g in seq:
        g_static.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    _same(c.bits(), e.bits(), "replay")
    assert torch.equal(c.guard.view(torch.int64), e.guard.view(torch.int64))
    norm, clip, sk, ap = c.guard.tolist()
    assert (sk, ap) == (1.0, 2.0) and clip < 0.01 and c.state[0].item() == 2


# ----------------------------------------------------------------------------- model level
_SMALL = dict(ngf=8, ndf=8, n_blocks=2)
_CASES = {"reference-f32": dict(dtype="f32"), "reference-bf16": dict(dtype="bf16"),
          "cycle-f32": dict(dtype="f32", cycle=True), "cycle-bf16": dict(dtype="bf16", cycle=True)}


def _feed(m, step=0, mask_scale=1.0, size=128):
    m.real_A, m.seg_A, mask = _rand_inputs(1, size, size, m.discriminator, 300 + 2 * step)
    m.mask_A = mask * mask_scale
    if m.cycle:
        m.real_B, m.seg_B, mask = _rand_inputs(1, size, size, m.discriminator, 301 + 2 * step)
        m.mask_B = mask * mask_scale


def _train_state(m):
    return [t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.iterations)]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _optimizers(m):
    return [m.g_optim, m.d_optim] + ([m.g_optim_BA, m.d_optim_B] if m.cycle else [])


@pytest.mark.parametrize("case", list(_CASES))
def test_model_guard_is_invisible_while_the_gradient_is_finite_and_under_the_bound(sg, case):
    """clip_grad_norm = 1e30 + skip_nonfinite: one train_step leaves every network's parameters, Adam slots and step counter
    bitwise as a model built without the options, and the records hold that step's norms."""
    kw = dict(_SMALL, **_CASES[case])
    plain = sg.sggan(sg.default_args(**kw))
    guarded = sg.sggan(sg.default_args(clip_grad_norm=1e30, skip_nonfinite=True, **kw))
    assert not plain.guarded and guarded.guarded and all(o.clip_norm == 1e30 and o.skip_nonfinite for o in _optimizers(guarded))
    assert all(o.clip_norm is None and not o.skip_nonfinite for o in _optimizers(plain))
    _feed(plain); _feed(guarded)
    plain.train_step(); guarded.train_step()
    for i, (x, y) in enumerate(zip(_train_state(plain), _train_state(guarded))):
        assert torch.equal(_bits(x), _bits(y)), (case, i)
    assert all(n.P._guard is None for n in plain.networks())
    stats = guarded.grad_stats()
    assert list(stats) == (["G", "D", "G_BA", "D_B"] if guarded.cycle else ["G", "D"])
    for name, st in stats.items():
        # (the reference-mode discriminator's gradient is exactly 0 at 128x128: its last normalised map is 1x1, so every logit
        # is the class bias -- 0 -- and the real and fake terms of the loss cancel)
        assert st["clip"] == 1.0 and st["skipped"] == 0 and st["applied"] == 1 and 0.0 <= st["norm"] < float("inf")
        assert st["norm"] > 0.0 or (name == "D" and not guarded.cycle)
    P = guarded.generator.P
    assert abs(stats["G"]["norm"] - float(P.grad.double().norm())) <= 1e-9 * stats["G"]["norm"]


@pytest.mark.parametrize("case", list(_CASES))
def test_nan_written_between_backward_and_update_skips_that_network_only(sg, case):
    """The step taken apart, eagerly, with the drop-in pieces (tests/test_gpu_step.py::test_dropin_callables_and_autograd's
    tape-style use): forward through generator(x) and discriminator([fake, mask]), backward, then -- between backward and
    update -- one element of one of the generator's gradients is overwritten with NaN, and every optimizer's
    apply_gradients(zip(grads, variables)) is called.  The generator keeps every bit of its parameters, Adam slots and step
    counter and counts one skip; every other network is updated (parameters, both slots and counter move: the loss below gives
    each network a non-zero gradient at 128x128, where the discriminator hands no gradient to its input)."""
    m = sg.sggan(sg.default_args(skip_nonfinite=True, **dict(_SMALL, **_CASES[case])))
    _feed(m)
    pairs = [(m.generator, m.discriminator, m.real_A, m.mask_A)]
    if m.cycle:
        pairs.append((m.generator_BA, m.discriminator_B, m.real_B, m.mask_B))
    for net in m.networks():
        net.requires_grad_(True)
    for G, D, real, mask in pairs:
        fake = G(real)
        out = D([fake, mask.cuda()])
        (((out - 1.0) ** 2).mean() + fake.abs().mean()).backward()
    grads = {net: [v.grad for v in net.trainable_variables] for net in m.networks()}
    assert all(g is not None and torch.isfinite(g).all() for gs in grads.values() for g in gs)
    assert all(any(g.abs().max() > 0 for g in gs) for gs in grads.values())
    s1 = _train_state(m)
    poisoned = grads[m.generator][len(grads[m.generator]) // 2]
    poisoned.view(-1)[poisoned.numel() // 2] = float("nan")                                # between backward and update
    for opt in _optimizers(m):
        opt.apply_gradients(zip(grads[opt.net], opt.net.trainable_variables))
    s2 = _train_state(m)
    for k, net in enumerate(m.networks()):
        same = [torch.equal(_bits(x), _bits(y)) for x, y in zip(s1[4 * k:4 * k + 4], s2[4 * k:4 * k + 4])]
        assert same == ([True] * 4 if net is m.generator else [False] * 4), (case, k, same)
    stats = m.grad_stats()
    assert (stats["G"]["skipped"], stats["G"]["applied"]) == (1, 0) and not math.isfinite(stats["G"]["norm"])
    assert all((st["skipped"], st["applied"]) == (0, 1) and 0.0 < st["norm"] < float("inf") for name, st in stats.items() if name != "G")
    assert m.generator.P.step_count == 0 and m.discriminator.P.step_count == 1


@pytest.mark.parametrize("case,size", [("reference-f32", 256), ("reference-bf16", 256), ("cycle-f32", 128), ("cycle-bf16", 128)])
def test_recorded_step_clips_at_replay_time(sg, case, size):
    """A guarded step recorded into HIP graphs and replayed; then masks 1000 times larger are written into the input buffers
    (the mask multiplies the discriminator's class logits, so its gradients grow with it; images would not do: instance norm
    makes the step invariant to their scale).  The replay of the SAME recording clips: grad_stats shows clip < 1 for the
    discriminator where the steps before show 1.  (Reference mode runs at 256x256: at 128x128 its discriminator's logits are
    the class biases whatever the input, and its gradient is 0 whatever the mask.)"""
    kw = dict(_SMALL, **_CASES[case])
    probe = sg.sggan(sg.default_args(clip_grad_norm=1e30, **kw))
    _feed(probe, size=size)
    probe.train_step()
    usual = probe.grad_stats()["D"]["norm"]
    assert usual > 0.0
    m = sg.sggan(sg.default_args(clip_grad_norm=8.0 * usual, graph=True, **kw))
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        for step in range(2):
            _feed(m, step, size=size)
            m.train_step()
            st = m.grad_stats()["D"]
            assert st["clip"] == 1.0 and st["applied"] == step + 1 and st["norm"] < 8.0 * usual, (step, st)   # (the warm-up step counted as none)
        prog = m._program
        assert prog is not None
        _feed(m, 2, mask_scale=1000.0, size=size)
        m.train_step()
    assert m._program is prog                                                              # no re-record
    st = m.grad_stats()["D"]
    print(f"[{case}] D gradient norm {usual:.3e} on the probe step, {st['norm']:.3e} with the masks x 1000: clip {st['clip']:.3e}")
    assert st["clip"] < 1.0 and st["norm"] > 8.0 * usual and (st["skipped"], st["applied"]) == (0, 3)
    assert st["clip"] == float(np.float32(float(np.float32(8.0 * usual)) / st["norm"]))


@pytest.mark.parametrize("case", list(_CASES))
def test_counters_survive_save_and_load(sg, case, tmp_path):
    kw = dict(_SMALL, **_CASES[case])
    m = sg.sggan(sg.default_args(skip_nonfinite=True, **kw))
    _feed(m)
    m.train_step()
    m.discriminator.P.grad[0] = float("inf")
    m._apply_gradients(*[(o, None) for o in _optimizers(m)])
    want = {k: (v["skipped"], v["applied"]) for k, v in m.grad_stats().items()}
    assert want["D"] == (1, 1) and want["G"] == (0, 2)
    m.save(str(tmp_path), 0)
    m2 = sg.sggan(sg.default_args(skip_nonfinite=True, **kw))
    assert m2.load(str(tmp_path))
    assert {k: (v["skipped"], v["applied"]) for k, v in m2.grad_stats().items()} == want
    for x, y in zip(_train_state(m), _train_state(m2)):
        assert torch.equal(_bits(x), _bits(y))
    # a checkpoint written without the options (no counters in it) loads, into a guarded model too
    sd = m.state_dict()
    for k in sd:
        assert sd[k].pop("guard") == list(want[k])
    m3 = sg.sggan(sg.default_args(skip_nonfinite=True, **kw))
    m3.load_state_dict(sd)
    assert all((v["skipped"], v["applied"]) == (0, 0) for v in m3.grad_stats().values())
    assert m3.discriminator.P.step_count == 1 and m3.generator.P.step_count == 2


def test_grad_scalars_follow_the_existing_ones(sg, tmp_path):
    """train() with --clip_grad_norm: per epoch, after 'Generator Loss' and 'Discriminator Loss', '<net> Grad Norm' and '<net>
    Skipped Updates' for G and D; without the flags the tags are the ones they were."""
    from sggan_amd.main import parse_args, synthetic_batches
    from sggan_amd.utils import SummarySink
    base = ["--img_height", "128", "--img_width", "128", "--ngf", "8", "--ndf", "8", "--batch_size", "1", "--steps_per_epoch", "1",
            "--dtype", "f32", "--epoch", "2"]
    def run(extra, name):
        a = parse_args(base + extra + ["--checkpoint_dir", str(tmp_path / name)])
        a.n_blocks = 2
        m = sg.sggan(a)
        sink = SummarySink()
        m.train(a, synthetic_batches(m, a), log=lambda *s: None, sink=sink)
        return m, sink
    m, sink = run(["--clip_grad_norm", "0.01"], "a")
    assert m.clip_grad_norm == 0.01 and not m.skip_nonfinite
    per_epoch = ["Generator Loss", "Discriminator Loss", "G Grad Norm", "G Skipped Updates", "D Grad Norm", "D Skipped Updates"]
    assert [r["tag"] for r in sink.records] == per_epoch * 2
    stats = m.grad_stats()
    last = {r["tag"]: r["value"] for r in sink.records if r["step"] == 1}
    assert last["G Grad Norm"] == stats["G"]["norm"] > 0.01 and last["D Skipped Updates"] == 0 and stats["G"]["clip"] < 1.0
    m, sink = run([], "b")
    assert [r["tag"] for r in sink.records] == per_epoch[:2] * 2 and not m.guarded


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
def test_dp_world1_with_clipping_is_bit_identical_to_the_plain_process(cycle):
    """tests/test_gpu_dp.py's world-1 run over RCCL with clip_grad_norm on (at a bound every network exceeds), at that test's
    256x256: the guard measures the buffer after the all-reduce's wait, eager and between HIP-graph segments; parameters, Adam
    slots, losses and the guard records equal the model without data parallelism, bit for bit."""
    import torch.distributed as dist
    import sggan_amd as sg
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        states = []
        for dp, graph in ((False, False), (True, False), (True, True)):
            m = sg.sggan(sg.default_args(dtype="f32", cycle=cycle, graph=graph, clip_grad_norm=1e-2, **_SMALL))
            if dp:
                m.enable_data_parallel()
            with warnings.catch_warnings(record=True):
                warnings.simplefilter("always")
                for step in range(2):
                    _feed(m, step, size=256)
                    m.train_step()
            stats = m.grad_stats()
            assert all(st["clip"] < 1.0 and (st["skipped"], st["applied"]) == (0, 2) for st in stats.values()), stats
            states.append(_train_state(m) + [m._loss.clone()] + [n.P._guard.clone().view(torch.int64) for n in m.networks()])
        for other in states[1:]:
            for i, (x, y) in enumerate(zip(states[0], other)):
                assert torch.equal(_bits(x), _bits(y)), i
    finally:
        dist.destroy_process_group()
