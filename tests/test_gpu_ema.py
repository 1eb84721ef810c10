"""GPU tests of the generator weight average (sgg_adam_ema / sgg_swap_f32, --ema_decay).

The reference for theta, m, v, iterations and the guard record is the existing entry point -- sgg_adam_iter, sgg_adam_sched,
sgg_adam_guard -- on the same inputs: the same f32 arithmetic, so those comparisons are BITWISE.  The reference for the
average is the float64 statement in tests/ema_oracle.py, fed the kernel's own f32 parameter sequence and the f32 d_t, at
the bound derived in test_average_against_the_float64_oracle.  Sizes sit at the edges of the update kernel's walk (16-byte
groups, the scalar tail, a partial chunk, several chunks of C elements), not at the networks' own sizes."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from tests import ema_oracle as E
from tests.test_gpu_grad_guard import _CASES, _SMALL, _bits, _feed, _free_port, _optimizers, _train_state

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-7
C = 2048
SIZES = [1, 3, 4, 5, 1020, 1023, 1024, 1028, C - 4, C, C + 4, 3 * C + 13]
K_STEPS = 12
U32 = 2.0 ** -24                                # unit roundoff of f32


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    import sggan_amd.kernels, sggan_amd.main  # noqa: F401,E401
    assert sggan_amd.kernels.EMA_CHUNK == C
    return sggan_amd


@functools.lru_cache(maxsize=None)
def _problem(n):
    """theta0, ema0 and K_STEPS gradients (host f32 tensors; generated once per size, never written)."""
    g = torch.Generator().manual_seed(4000 + n % 997)
    return torch.randn(n, generator=g), torch.randn(n, generator=g), tuple(torch.randn(n, generator=g) * 0.1 for _ in range(K_STEPS))


@functools.lru_cache(maxsize=None)
def _norm(n, k):
    return float(_problem(n)[2][k].double().norm())


class _Slots:
    def __init__(self, sg, n):
        theta0, ema0, _ = _problem(n)
        self.K = sg.kernels
        self.theta, self.ema = theta0.clone().cuda(), ema0.clone().cuda()
        self.m, self.v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        self.state = torch.zeros(2, dtype=torch.int64, device="cuda")
        self.ema_state = torch.full((2,), -1.0, device="cuda")
        self.guard = torch.zeros(4, dtype=torch.float64, device="cuda")
        self.ws = self.K.grad_guard_workspace(n, "cuda")

    def ema_step(self, g, decay, sched=None, guarded=False, max_norm=0.0, grad_scale=1.0):
        self.K.adam_ema(self.theta, g, self.m, self.v, self.ema, self.state, self.ema_state, decay, sched, LR, B1, B2, EPS, grad_scale,
                        self.guard if guarded else None, self.ws if guarded else None, max_norm)

    def plain(self, g, sched=None):
        if sched is None:
            self.K.adam_iter(self.theta, g, self.m, self.v, self.state, LR, B1, B2, EPS, 1.0)
        else:
            self.K.adam_sched(self.theta, g, self.m, self.v, self.state, sched, LR, B1, B2, EPS, 1.0)

    def guarded(self, g, sched=None, max_norm=0.0):
        self.K.adam_guard(self.theta, g, self.m, self.v, self.state, self.guard, self.ws, sched, LR, B1, B2, EPS, 1.0, max_norm)

    def bits(self, ema=False):
        out = [self.theta.view(torch.int32).clone(), self.m.view(torch.int32).clone(), self.v.view(torch.int32).clone(),
               self.state[0:1].clone()]
        if ema:
            out += [self.ema.view(torch.int32).clone(), self.ema_state.view(torch.int32).clone()]
        return out


_NAMES = ("theta", "m", "v", "iterations", "ema", "ema_state")


def _same(a, b, what):
    assert len(a) == len(b)
    for name, x, y in zip(_NAMES, a, b):
        assert torch.equal(x, y), (what, name)


# ----------------------------------------------------------------------------- flat buffers
@pytest.mark.parametrize("n", SIZES)
def test_plain_paths_are_bitwise_the_existing_updates(sg, n):
    """guarded = 0: theta, m, v and iterations after each of three steps equal sgg_adam_iter's and, with a schedule whose third
    step decays, sgg_adam_sched's -- bit for bit."""
    theta0, _, grads = _problem(n)
    for sched_host in (None, (1, 1, 4)):
        sched = None if sched_host is None else torch.tensor(sched_host, dtype=torch.int64, device="cuda")
        a, b = _Slots(sg, n), _Slots(sg, n)
        for it in range(3):
            g = grads[it].cuda()
            a.ema_step(g, 0.999, sched)
            b.plain(g, sched)
            _same(a.bits(), b.bits(), (n, sched_host, it))
        assert a.state[0].item() == 3 and a.guard.tolist() == [0.0] * 4          # (no guard record without `guarded`)
    assert not torch.equal(a.theta.cpu(), theta0)                                # (the steps did move something)


@pytest.mark.parametrize("n", SIZES)
def test_guarded_path_is_bitwise_the_guarded_update(sg, n):
    """guarded = 1, without a bound, under one and above one (half the gradient's norm: clipped), with and without a schedule:
    theta, m, v, iterations and guard[0..3] equal sgg_adam_guard's, bit for bit, after each of three steps."""
    _, _, grads = _problem(n)
    for sched_host in (None, (1, 1, 4)):
        sched = None if sched_host is None else torch.tensor(sched_host, dtype=torch.int64, device="cuda")
        for factor in (0.0, 2.0, 0.5):
            a, b = _Slots(sg, n), _Slots(sg, n)
            for it in range(3):
                g = grads[it].cuda()
                max_norm = float(np.float32(factor * _norm(n, it)))
                a.ema_step(g, 0.999, sched, guarded=True, max_norm=max_norm)
                b.guarded(g, sched, max_norm=max_norm)
                _same(a.bits(), b.bits(), (n, sched_host, factor, it))
                assert torch.equal(a.guard.view(torch.int64), b.guard.view(torch.int64)), (n, sched_host, factor, it)
            clip, skipped, applied = a.guard.tolist()[1:]
            assert (skipped, applied) == (0.0, 3.0) and ((clip < 1.0) if factor == 0.5 else (clip == 1.0))


@pytest.mark.parametrize("decay", [0.5, 0.999])
@pytest.mark.parametrize("n", SIZES)
def test_average_against_the_float64_oracle(sg, n, decay):
    """K_STEPS = 12 steps (for D = 0.5 the ramp ends at t = 8, so both regimes run; for D = 0.999 all twelve are on the ramp),
    plain and guarded.  The oracle gets the kernel's own f32 theta after every step and the f32 (d_t, 1 - d_t).

    Bound, derived: per element and step the kernel rounds three times in f32 -- d_t * ema, (1 - d_t) * theta, their sum --
    each by at most 2^-24 times its result, and every result is at most max_abs (1 + 2^-23) in magnitude, max_abs being the
    largest |ema| or |theta| on the way (d_t + (1 - d_t) <= 1 + 2^-25).  The error carried over is multiplied by d_t < 1, so
    it does not grow: |ema - oracle| <= 3 k 2^-24 max_abs after k steps (the 2^-23 excess is below one part in 10^6 of that
    and the oracle's own float64 rounding below one in 10^8; neither is added).
    ema_state is (d_t, 1 - d_t) exactly after every step; two runs give the same bits."""
    _, ema0, grads = _problem(n)
    runs = []
    for guarded in (False, True, False):
        s = _Slots(sg, n)
        thetas = []
        for it in range(K_STEPS):
            s.ema_step(grads[it].cuda(), decay, guarded=guarded)
            d, omd = E.decay_f32(decay, it + 1)
            assert s.ema_state.cpu().numpy().tolist() == [d, omd], (n, decay, it)
            thetas.append(s.theta.cpu().numpy())
        runs.append((s.bits(ema=True), thetas))
    _same(runs[0][0], runs[2][0], (n, decay, "second run"))
    _same(runs[0][0], runs[1][0], (n, decay, "guarded run"))
    want, max_abs = E.ema_run(ema0.numpy(), runs[0][1], decay)
    got = runs[0][0][4].view(torch.float32).cpu().numpy().astype(np.float64)
    err, bound = float(np.abs(got - want).max()), 3 * K_STEPS * U32 * max_abs
    print(f"n = {n} D = {decay}: max |ema - oracle| = {err:.3e}, bound {bound:.3e} (max_abs {max_abs:.3f})")
    assert err <= bound
    assert E.decay_f32(decay, K_STEPS)[0] == np.float32(decay if decay == 0.5 else 13.0 / 22.0)
    assert not np.array_equal(got, ema0.numpy().astype(np.float64))                        # (the average did move)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_gradient_keeps_the_average_and_the_next_step_counts_on(sg, n, bad):
    """guarded = 1: after one applied step a gradient with one non-finite element -- first, last and middle position in turn --
    leaves theta, m, v, ema, ema_state and iterations with every bit and counts a skip.  The finite step after them applies
    with t = 2, not 2 + skips: ema_state is (d_2, 1 - d_2) and everything equals two applied steps of the plain path."""
    _, _, grads = _problem(n)
    a, b = _Slots(sg, n), _Slots(sg, n)
    a.ema_step(grads[0].cuda(), 0.999, guarded=True); b.ema_step(grads[0].cuda(), 0.999)
    before = a.bits(ema=True)
    g = grads[1].clone().cuda()
    positions = sorted({0, n // 2, n - 1, n - n % 4 - 1 if n >= 4 else 0})
    for k, pos in enumerate(positions):
        keep = g[pos].item()
        g[pos] = bad
        a.ema_step(g, 0.999, guarded=True, max_norm=0.0 if k % 2 == 0 else 1e-3)
        _same(a.bits(ema=True), before, (n, pos))
        assert a.guard.tolist()[2:] == [float(k + 1), 1.0], (n, pos)
        g[pos] = keep
    a.ema_step(grads[2].cuda(), 0.999, guarded=True); b.ema_step(grads[2].cuda(), 0.999)
    _same(a.bits(ema=True), b.bits(ema=True), (n, "the step after the skips"))
    d, omd = E.decay_f32(0.999, 2)
    assert a.state[0].item() == 2 and a.ema_state.cpu().numpy().tolist() == [d, omd]


def _payloads(n, seed):
    """Random 32-bit patterns: about one in 256 is a NaN or Inf, each with its own payload; plus the canonical ones."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([0x7fc00001, -4194303, 0x7f800000, -8388608, 0x7fffffff, 0x00000001], dtype=torch.int64).to(torch.int32)
    k = min(n, special.numel())
    x[n - k:] = special[:k]
    return x


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_every_bit(sg, n):
    K = sg.kernels
    a0, b0 = _payloads(n, 1), _payloads(n, 2)
    assert torch.isnan(a0.view(torch.float32)).any() or n < 1
    pad = 8                                                                       # a guard band behind each buffer: not touched
    A_, B_ = torch.full((n + pad,), 7, dtype=torch.int32).cuda(), torch.full((n + pad,), 9, dtype=torch.int32).cuda()
    a, b = A_[:n].view(torch.float32), B_[:n].view(torch.float32)
    A_[:n] = a0.cuda(); B_[:n] = b0.cuda()
    K.swap_(a, b)
    assert torch.equal(A_[:n].cpu(), b0) and torch.equal(B_[:n].cpu(), a0)
    assert A_[n:].tolist() == [7] * pad and B_[n:].tolist() == [9] * pad
    K.swap_(a, b)
    assert torch.equal(A_[:n].cpu(), a0) and torch.equal(B_[:n].cpu(), b0)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_update_replays_from_a_captured_graph(sg, guarded):
    """One warm-up call, then sgg_adam_ema captured once and replayed 4 times with other gradients in the static buffer: equal to
    5 eager calls bitwise, ema and ema_state included -- the ramp follows the device counter, not the captured arguments."""
    n = 3 * C + 13
    _, _, grads = _problem(n)
    e = _Slots(sg, n)
    for it in range(5):
        e.ema_step(grads[it].cuda(), 0.5, guarded=guarded)
    c = _Slots(sg, n)
    g_static = grads[0].clone().cuda()
    c.ema_step(g_static, 0.5, guarded=guarded)
    torch.cuda.synchronize()
    after_warmup = c.bits(ema=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.ema_step(g_static, 0.5, guarded=guarded)
    _same(c.bits(ema=True), after_warmup, "capturing ran nothing")
    for it in range(1, 5):
        g_static.copy_(grads[it])
        graph.replay()
    torch.cuda.synchronize()
    _same(c.bits(ema=True), e.bits(ema=True), "replay")
    assert torch.equal(c.guard.view(torch.int64), e.guard.view(torch.int64))
    assert c.state[0].item() == 5 and c.ema_state.cpu().numpy().tolist() == list(E.decay_f32(0.5, 5))


# ----------------------------------------------------------------------------- model level
_MODEL_CASES = dict(_CASES, **{"unet-f32": dict(dtype="f32", use_resnet=False),
                               "cycle-unet-bf16": dict(dtype="bf16", cycle=True, use_resnet=False)})
D_MODEL = 0.5


def _model(sg, case, **over):
    return sg.sggan(sg.default_args(**dict(_SMALL, **_MODEL_CASES[case]), **over))


def _ema_state(m):
    return [t.clone() for n in m._ema_nets() for t in (n.P.ema, n.P._ema_state)]


def _assert_same(xs, ys, what):
    assert len(xs) == len(ys)
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert torch.equal(_bits(x), _bits(y)), (what, i)


@pytest.mark.parametrize("case", list(_MODEL_CASES))
def test_model_average_is_invisible_to_training_and_tracks_the_oracle(sg, case):
    """Three train steps with ema_decay set: every network's parameters, Adam slots, step counter and both losses are bitwise
    those of the same model without it; only the generators carry an average; it differs from the parameters and is the
    oracle's average of the recorded parameter sequence (started from the initial parameters) at 3 k 2^-24 max_abs, k = 3."""
    plain, m = _model(sg, case), _model(sg, case, ema_decay=D_MODEL)
    assert plain.ema_decay is None and m.ema_decay == D_MODEL
    assert [o.ema_decay for o in _optimizers(m)] == ([D_MODEL, None, D_MODEL, None] if m.cycle else [D_MODEL, None])
    assert all(n.P.ema is None for n in plain.networks()) and m.discriminator.P.ema is None
    gens = m._ema_nets()
    assert len(gens) == (2 if m.cycle else 1)
    start = [n.P.flat.cpu().numpy() for n in gens]
    assert all(np.array_equal(n.P.ema.cpu().numpy(), s) for n, s in zip(gens, start))
    seq = [[] for _ in gens]
    for step in range(3):
        _feed(plain, step); _feed(m, step)
        plain.train_step(); m.train_step()
        for k, n in enumerate(gens):
            seq[k].append(n.P.flat.cpu().numpy())
    _assert_same(_train_state(plain) + [plain._loss.clone()], _train_state(m) + [m._loss.clone()], case)
    for n, s0, thetas in zip(gens, start, seq):
        got = n.P.ema.cpu().numpy()
        assert not np.array_equal(got, thetas[-1])
        want, max_abs = E.ema_run(s0, thetas, D_MODEL)
        assert np.abs(got.astype(np.float64) - want).max() <= 3 * 3 * U32 * max_abs
        assert n.P._ema_state.cpu().numpy().tolist() == list(E.decay_f32(D_MODEL, 3)) and n.P.step_count == 3


def test_bad_decay_and_models_without_an_average_are_refused(sg):
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            _model(sg, "reference-f32", ema_decay=bad)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with _model(sg, "reference-f32").ema_weights():
            pass


@pytest.mark.parametrize("case", list(_MODEL_CASES))
def test_ema_weights_context_swaps_in_the_average_and_hands_the_weights_back(sg, case):
    """Inside ema_weights() each generator's output is that of a fresh generator loaded with P.export(buf=ema); after exit flat
    and ema have their bits back, and the next step -- eager, then replayed from HIP graphs recorded BEFORE another visit to the
    context -- leaves the model bitwise where its twin is, which never entered."""
    m, twin = _model(sg, case, ema_decay=D_MODEL), _model(sg, case, ema_decay=D_MODEL)
    fresh = _model(sg, case)
    for step in range(2):
        _feed(m, step); _feed(twin, step)
        m.train_step(); twin.train_step()
    full = lambda mod: _train_state(mod) + _ema_state(mod) + [mod._loss.clone()]
    _assert_same(full(m), full(twin), "before")
    x = torch.rand((1, 128, 128, 3), generator=torch.Generator().manual_seed(77)).cuda()
    pairs = list(zip(m._ema_nets(), fresh._ema_nets()))

    def visit():
        before = full(m)
        trained = [G(x).clone() for G, _ in pairs]
        for (G, F) in pairs:
            F.P.load(G.P.export(buf=G.P.ema))
        with m.ema_weights() as inside:
            assert inside is m
            for (G, F), t in zip(pairs, trained):
                out = G(x)
                assert torch.equal(out, F(x)) and (m.dtype != torch.float32 or not torch.equal(out, t))
        _assert_same(full(m), before, "after the context")
        for (G, _), t in zip(pairs, trained):
            assert torch.equal(G(x), t)                                            # (and the packed operands were rebuilt)

    visit()
    _feed(m, 2); _feed(twin, 2)
    m.train_step(); twin.train_step()
    _assert_same(full(m), full(twin), "eager step after the context")
    m.enable_graph(); twin.enable_graph()
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        _feed(m, 3); _feed(twin, 3)
        m.train_step(); twin.train_step()                                          # records, then replays
        _assert_same(full(m), full(twin), "first graph step")
        prog = m._program
        visit()
        _feed(m, 4); _feed(twin, 4)
        m.train_step(); twin.train_step()
    assert m._program is prog and prog is not None
    _assert_same(full(m), full(twin), "replayed step after the context")
    assert m.generator.P.step_count == 5 and m.generator.P._ema_state[0].item() == float(E.decay_f32(D_MODEL, 5)[0])


@pytest.mark.parametrize("case", list(_CASES))
def test_average_survives_save_and_load(sg, case, tmp_path, capsys):
    m = _model(sg, case, ema_decay=D_MODEL)
    for step in range(2):
        _feed(m, step)
        m.train_step()
    m.save(str(tmp_path / "ema"), 0)
    m2 = _model(sg, case, ema_decay=D_MODEL, seed=23)
    capsys.readouterr()
    assert m2.load(str(tmp_path / "ema")) and capsys.readouterr().out == ""
    _assert_same(_train_state(m), _train_state(m2), "state")
    _assert_same([n.P.ema for n in m._ema_nets()], [n.P.ema for n in m2._ema_nets()], "ema")
    assert not torch.equal(m2.generator.P.ema, m2.generator.P.flat)
    # the same checkpoint into a model without the average: the key is ignored
    m3 = _model(sg, case, seed=23)
    assert m3.load(str(tmp_path / "ema")) and all(n.P.ema is None for n in m3.networks())
    _assert_same(_train_state(m), _train_state(m3), "plain model")
    # a checkpoint written before the average existed: it starts from the loaded weights, said once
    m3.save(str(tmp_path / "plain"), 0)
    m4 = _model(sg, case, ema_decay=D_MODEL, seed=29)
    assert m4.load(str(tmp_path / "plain"))
    assert capsys.readouterr().out.count("checkpoint without a weight average") == 1      # (once, not per generator)
    for n, src in zip(m4._ema_nets(), m._ema_nets()):
        assert torch.equal(_bits(n.P.ema), _bits(n.P.flat)) and torch.equal(_bits(n.P.flat), _bits(src.P.flat))


def test_test_during_train_runs_on_the_average_and_logs_the_decay(sg, tmp_path):
    """test_during_train on two synthetic samples: the returned images are the ones the generator gives inside ema_weights(),
    computed here by hand, not the trained weights' -- and the sink holds the four scalars a run without the flag logs, in
    their order, followed by 'EMA Decay' = the last d_t.  The trained weights are back afterwards."""
    from sggan_amd.main import parse_args, synthetic_test_samples
    from sggan_amd.utils import SummarySink, convert_image_dtype_uint8, get_img
    base = ["--img_height", "128", "--img_width", "128", "--ngf", "8", "--ndf", "8", "--batch_size", "1", "--dtype", "f32"]

    def build(extra):
        a = parse_args(base + extra)
        a.n_blocks, a.test_dir = 2, None
        m = sg.sggan(a)
        for step in range(3):
            _feed(m, step)
            m.train_step()
        return a, m

    def by_hand(m, a):
        return np.concatenate([get_img(m.generator(torch.as_tensor(convert_image_dtype_uint8(np.asarray(s[1])[None])).to(m.device)), [1, 1])
                               for s in synthetic_test_samples(a, 2)()], axis=0)

    a, m = build(["--ema_decay", str(D_MODEL)])
    assert m.ema_decay == D_MODEL
    before = _train_state(m) + _ema_state(m)
    sink = SummarySink()
    images, score = m.test_during_train(5, a, synthetic_test_samples(a, 2)(), sink)
    _assert_same(_train_state(m) + _ema_state(m), before, "after the test pass")
    with m.ema_weights():
        want = by_hand(m, a)
    assert images.shape[0] == 2 and np.array_equal(images, want)
    assert not np.array_equal(want, by_hand(m, a))                                 # (the trained weights give other images)
    usual = ["Overall Accuracy", "Mean Accuracy", "Frequency Weighted Accuracy", "Mean IoU"]
    assert [r["tag"] for r in sink.records] == usual + ["EMA Decay"] and all(r["step"] == 5 for r in sink.records)
    assert sink.records[-1]["value"] == float(E.decay_f32(D_MODEL, 3)[0]) and m.generator.P.step_count == 3

    a0, m0 = build([])
    sink0 = SummarySink()
    images0, _ = m0.test_during_train(5, a0, synthetic_test_samples(a0, 2)(), sink0)
    assert [r["tag"] for r in sink0.records] == usual and m0.ema_decay is None
    assert np.array_equal(images0, by_hand(m0, a0))
    # --phase test: the translations of the checkpoint's average
    m.save(str(tmp_path / "ck"), 0)
    a.checkpoint_dir, a.test_dir = str(tmp_path / "ck"), str(tmp_path / "out")
    m5 = sg.sggan(a)
    outs = m5.test(a, synthetic_test_samples(a, 2)(), log=lambda *s: None)
    with m.ema_weights():
        for s, out in zip(synthetic_test_samples(a, 2)(), outs):
            x = torch.as_tensor(convert_image_dtype_uint8(np.asarray(s[1], dtype=np.float32)[None])).to(m.device)
            assert torch.equal(out, m.generator(x))


# ----------------------------------------------------------------------------- data parallel
def _dp_worker(port, out):
    """A fresh process (the one that initialises RCCL): the cycle model with ema_decay, two steps, single-process / world 1
    eager / world 1 under HIP graphs."""
    try:
        import torch.distributed as dist
        import sggan_amd as sg
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        states = []
        for dp, graph in ((False, False), (True, False), (True, True)):
            m = sg.sggan(sg.default_args(dtype="f32", cycle=True, graph=graph, ema_decay=D_MODEL, **_SMALL))
            if dp:
                m.enable_data_parallel()
            with warnings.catch_warnings(record=True):
                warnings.simplefilter("always")
                for step in range(2):
                    _feed(m, step)
                    m.train_step()
            states.append([_bits(t).cpu().numpy() for t in _train_state(m) + _ema_state(m) + [m._loss.clone()]])
        dist.destroy_process_group()
        out.put((states, None))
    except Exception:                                       # surfaced by the parent
        import traceback
        out.put((None, traceback.format_exc()))


def test_dp_world1_average_is_bit_identical_to_the_single_process_run():
    """Nothing is exchanged for the average: every rank applies the same update to it.  World 1 over RCCL, eager and with the
    collectives between HIP-graph segments (whose recording restores the average after its warm-up step): ema, ema_state,
    parameters, slots and losses equal the run without data parallelism, bit for bit."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_worker, args=(_free_port(), q))
    p.start()
    states, err = q.get(timeout=300)
    p.join(60)
    assert err is None, err
    assert p.exitcode == 0
    n_ema = 4                                               # (ema, ema_state) of two generators, in front of the losses
    for other in states[1:]:
        assert len(other) == len(states[0])
        for i, (x, y) in enumerate(zip(states[0], other)):
            assert np.array_equal(x, y), i
    ema, flat = states[0][-1 - n_ema], states[0][0]
    assert ema.shape == flat.shape and not np.array_equal(ema, flat)
