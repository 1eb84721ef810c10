"""GPU tests of the linear learning-rate decay evaluated on the device (sgg_adam_sched, --lr_decay).

The reference for the kernel is the existing entry point: sgg_adam_iter given the rate the host statement of the rule
(kernels.scheduled_lr) yields for that iteration -- both run the same device pow / sqrt on the same f32 rate, so every
comparison of that kind is BITWISE.  The model-level tests compare a model that decays on the device against one whose
optimizers get the same rates assigned by the host before every eager step."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import sggan_oracle as O
from tests.test_gpu_step import _rand_inputs

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-7
SCHED = (2, 1, 4)          # steps_per_epoch, epoch_step, epochs: 10 steps = 2 flat, 2 + 2 + 2 decayed (3/3, 2/3, 1/3), 2 clamped at 0
STEPS = 10
SIZES = [1, 255, 4099, (1 << 20) + 7]      # tail only, a part block, a multi-block tail, grid stride (2048 x 256 < n)


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    import sggan_amd.kernels, sggan_amd.main, sggan_amd.utils  # noqa: F401,E401
    return sggan_amd


@functools.lru_cache(maxsize=None)
def _problem(n):
    """theta0 and one fresh gradient per step (host f32 tensors; generated once per size, never written)."""
    g = torch.Generator().manual_seed(1000 + n % 997)
    theta = torch.randn(n, generator=g)
    grads = tuple(torch.randn(n, generator=g) * 0.1 for _ in range(STEPS))
    return theta, grads


def _slots(theta):
    return theta.clone().cuda(), torch.zeros_like(theta).cuda(), torch.zeros_like(theta).cuda(), torch.zeros(2, dtype=torch.int64, device="cuda")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("n", SIZES)
def test_adam_sched_is_bitwise_adam_iter_at_the_scheduled_rate(sg, n):
    K = sg.kernels
    theta0, grads = _problem(n)
    sched = torch.tensor(SCHED, dtype=torch.int64, device="cuda")
    ta, ma, va, sa = _slots(theta0)
    tb, mb, vb, sb = _slots(theta0)
    rates = []
    for it in range(STEPS):
        g = grads[it].cuda()
        lr_e = K.scheduled_lr(LR, it, *SCHED)
        rates.append(float(lr_e))
        before = (ta.clone(), ma.clone(), va.clone())
        K.adam_sched(ta, g, ma, va, sa, sched, LR, B1, B2, EPS)
        K.adam_iter(tb, g, mb, vb, sb, float(lr_e), B1, B2, EPS)
        for name, x, y in (("theta", ta, tb), ("m", ma, mb), ("v", va, vb)):
            assert torch.equal(_bits(x), _bits(y)), (n, it, name)
        assert sa[0].item() == sb[0].item() == it + 1
        if it >= 8:                                          # clamp: epochs - e <= 0 -> rate 0: theta stays, the slots still move
            assert lr_e == 0.0
            assert torch.equal(_bits(ta), _bits(before[0])), (n, it)
            assert not torch.equal(ma, before[1]) and not torch.equal(va, before[2]), (n, it)
        else:
            assert lr_e > 0.0 and (n == 1 or not torch.equal(ta, before[0])), (n, it)   # (one element may move by < 1/2 ulp)
    f = np.float32
    assert rates == [float(f(LR))] * 4 + [float(f(float(f(LR)) * 2 / 3))] * 2 + [float(f(float(f(LR)) * 1 / 3))] * 2 + [0.0, 0.0]


def _adam_tf_form_bound():
    """The bound tests/test_gpu_ops.py::test_adam_tf_form holds sgg_adam to, read from that file."""
    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_ops.py")).read()
    body = src[src.index("def test_adam_tf_form"):]
    return float(re.search(r"np\.abs\(tth\.detach\(\)\.cpu\(\)\.numpy\(\) - th\)\.max\(\) < ([0-9.eE+-]+)", body).group(1))


def test_adam_sched_against_the_float64_oracle(sg):
    """The same 10 steps against oracle.adam_tf in float64 with the float64 form of the rule (model.py:223 on
    epoch = iteration // steps_per_epoch, 0 past the last epoch), at test_adam_tf_form's bound."""
    K = sg.kernels
    bound = _adam_tf_form_bound()
    assert 0.0 < bound <= 2e-6
    n = 4099
    theta0, grads = _problem(n)
    sched = torch.tensor(SCHED, dtype=torch.int64, device="cuda")
    tt, tm, tv, st = _slots(theta0)
    th, m, v = theta0.double().numpy(), np.zeros(n), np.zeros(n)
    spe, step, epochs = SCHED
    for it in range(STEPS):
        e = it // spe
        lr64 = LR if e < step else LR * max(epochs - e, 0) / (epochs - step)
        th, m, v = O.adam_tf(th, grads[it].double().numpy(), m, v, it + 1, lr64, B1, B2, EPS)
        K.adam_sched(tt, grads[it].cuda(), tm, tv, st, sched, LR, B1, B2, EPS)
    err = np.abs(tt.cpu().numpy() - th).max()
    print(f"adam_sched vs float64 oracle after {STEPS} steps: max |theta - oracle| = {err:.3e} (bound {bound:.1e})")
    assert err < bound
    assert np.abs(tm.cpu().numpy() - m).max() < bound and np.abs(tv.cpu().numpy() - v).max() < bound


def test_schedule_written_after_capture_is_followed_by_the_replays(sg):
    """One adam_sched call captured with the "never decays" descriptor; {1, 1, 3} written into the descriptor afterwards; four
    replays == four eager calls with the descriptor set from the start, bitwise (rates lr, lr*2/2, lr*1/2, 0)."""
    K = sg.kernels
    n = 4099
    theta0, grads = _problem(n)
    # eager, descriptor set from the start (also loads the kernels before anything is captured)
    sched_e = torch.tensor((1, 1, 3), dtype=torch.int64, device="cuda")
    te, me, ve, se = _slots(theta0)
    for it in range(4):
        K.adam_sched(te, grads[it].cuda(), me, ve, se, sched_e, LR, B1, B2, EPS)
    # captured with "never decays"
    sched_g = torch.tensor((1, 0, 0), dtype=torch.int64, device="cuda")
    tg, mg, vg, sg_ = _slots(theta0)
    g_static = torch.zeros(n, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.adam_sched(tg, g_static, mg, vg, sg_, sched_g, LR, B1, B2, EPS)
    assert sg_[0].item() == 0 and torch.equal(tg.cpu(), theta0)          # capturing ran nothing
    sched_g.copy_(torch.tensor((1, 1, 3), dtype=torch.int64))
    for it in range(4):
        g_static.copy_(grads[it])
        graph.replay()
    torch.cuda.synchronize()
    for name, x, y in (("theta", tg, te), ("m", mg, me), ("v", vg, ve)):
        assert torch.equal(_bits(x), _bits(y)), name
    assert sg_[0].item() == se[0].item() == 4
    # and the schedule did act: without it the same four steps end elsewhere
    tn, mn, vn, sn = _slots(theta0)
    for it in range(4):
        K.adam_iter(tn, grads[it].cuda(), mn, vn, sn, LR, B1, B2, EPS)
    assert not torch.equal(tn, te) and torch.equal(mn, me)


# ----------------------------------------------------------------------------- model level
# the step configuration of tests/test_gpu_step.py's f32 small-step test (ngf 8, ndf 8, two blocks, 128x128), at batch 1
_SMALL = dict(ngf=8, ndf=8, n_blocks=2, dtype="f32")
_MODEL_SCHED = (1, 1, 3)                 # 4 steps: lr, lr*2/2, lr*1/2, 0
_CASES = {"reference": dict(), "cycle_paired": dict(cycle=True), "unet_cycle": dict(cycle=True, use_resnet=False)}


def _feed(m, step):
    m.real_A, m.seg_A, m.mask_A = _rand_inputs(1, 128, 128, m.discriminator, 300 + 2 * step)
    if m.cycle:
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(1, 128, 128, m.discriminator, 301 + 2 * step)


def _optimizers(m):
    return [m.g_optim, m.d_optim] + ([m.g_optim_BA, m.d_optim_B] if m.cycle else [])


def _train_state(m):
    return [t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.iterations)]


def _assert_same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(_bits(x), _bits(y)), (what, "network %d" % (i // 4), ("flat", "m", "v", "iterations")[i % 4])


@pytest.mark.parametrize("case", list(_CASES))
def test_model_decay_on_device_equals_host_assigned_rates(sg, case):
    """sggan(lr_decay=True) + set_lr_schedule(1, 1, 3) against the same model without lr_decay whose optimizers get
    learning_rate = scheduled_lr(base, step, 1, 1, 3) from the host before every eager step: all parameters and Adam slots of
    all networks bitwise equal after each of 4 steps.  Reference mode (2 optimizers, base 1e-3), the paired ResNet cycle step
    and the U-Net cycle step one network at a time (4 optimizers, base --lr)."""
    K = sg.kernels
    kw = dict(_SMALL, **_CASES[case])
    A_ = sg.sggan(sg.default_args(lr_decay=True, **kw))
    B_ = sg.sggan(sg.default_args(**kw))
    assert A_.lr_decay and not B_.lr_decay and B_._lr_sched is None
    assert A_.paired == (case == "cycle_paired" or not A_.cycle) and A_.arch == ("unet" if case == "unet_cycle" else "resnet")
    assert len({o.schedule.data_ptr() for o in _optimizers(A_)}) == 1 and A_._lr_sched.tolist() == [1, 0, 0]
    A_.set_lr_schedule(*_MODEL_SCHED)
    base = [o.learning_rate for o in _optimizers(B_)]
    assert base == [o.learning_rate for o in _optimizers(A_)] == [2e-4 if A_.cycle else 1e-3] * len(base)
    prev = None
    for step in range(4):
        _feed(A_, step); _feed(B_, step)
        for o, lr0 in zip(_optimizers(B_), base):
            o.learning_rate = float(K.scheduled_lr(lr0, step, *_MODEL_SCHED))
        A_.train_step(); B_.train_step()
        sa, sb = _train_state(A_), _train_state(B_)
        _assert_same(sa, sb, (case, step))
        if step == 3:                                        # rate 0: no parameter moved
            assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(sa[0::4], prev[0::4]))
        prev = sa
    assert [o.learning_rate for o in _optimizers(A_)] == base    # the base rates were never touched
    with pytest.raises(RuntimeError):
        B_.set_lr_schedule(*_MODEL_SCHED)


@pytest.mark.parametrize("case", ["reference", "cycle_paired"])
def test_model_decay_under_graph_replay_equals_eager(sg, case):
    """graph=True against eager over the same 4 steps, the descriptor written after the first (recording) step: bitwise."""
    def run(graph):
        m = sg.sggan(sg.default_args(lr_decay=True, graph=graph, **dict(_SMALL, **_CASES[case])))
        out = []
        for step in range(4):
            _feed(m, step)
            m.train_step()
            if step == 0:
                m.set_lr_schedule(*_MODEL_SCHED)
            out.append(_train_state(m) + [m._loss.clone()])
        return m, out
    me, eager = run(False)
    mg, graph = run(True)
    assert mg._program is not None and me._program is None
    for step, (a, b) in enumerate(zip(eager, graph)):
        _assert_same(a[:-1], b[:-1], (case, step))
        assert torch.equal(a[-1], b[-1]), step
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(graph[3][0:-1:4], graph[2][0:-1:4]))   # the replayed step 4 ran at rate 0


class _Interrupt(Exception):
    pass


def test_decay_continues_after_resume(sg, tmp_path):
    """--lr_decay --epoch 4 --epoch_step 1, 2 steps per epoch.  A run interrupted after 2 epochs (train() saves in ``finally``)
    and continued by a fresh model with --continue_train ends bit for bit where the uninterrupted 4-epoch run ends: the
    schedule's epoch is iterations // steps_per_epoch, and ``iterations`` comes back with the Adam slots -- the resumed loop
    counts its epochs from 0 again, the decay does not.  (tests/test_gpu_next_rows.py::test_train_loop_checkpoint_resume's method;
    the runs keep --epoch 4, which the rule reads, and stop by interruption instead.)"""
    argv = ["--epoch", "4", "--epoch_step", "1", "--lr_decay", "--batch_size", "1", "--img_height", "128", "--img_width", "128",
            "--ngf", "8", "--ndf", "8", "--dtype", "f32", "--steps_per_epoch", "2", "--dataset_dir", "unit"]
    def args(ckpt, **over):
        a = sg.main.parse_args(argv + ["--checkpoint_dir", str(tmp_path / ckpt)])
        a.n_blocks = 2
        for k, v in over.items():
            setattr(a, k, v)
        return a
    a0 = args("ck")
    m0 = sg.sggan(a0)
    assert m0.lr_decay
    hist = m0.train(a0, sg.main.synthetic_batches(m0, a0), log=lambda s: None)
    assert len(hist) == 4 and m0.generator.P.step_count == 8 and m0._lr_sched.tolist() == [2, 1, 4]

    def two_epochs(source, first):
        def batches(ep):
            if ep == 2:
                raise _Interrupt()
            return source(first + ep)
        return batches
    a1 = args("ck2")
    m1 = sg.sggan(a1)
    with pytest.raises(_Interrupt):
        m1.train(a1, two_epochs(sg.main.synthetic_batches(m1, a1), 0), log=lambda s: None)
    assert m1.generator.P.step_count == 4
    a2 = args("ck2", continue_train=True)
    m2 = sg.sggan(a2)
    with pytest.raises(_Interrupt):
        m2.train(a2, two_epochs(sg.main.synthetic_batches(m2, a2), 2), log=lambda s: None)
    for x, y in zip(m0.networks(), m2.networks()):
        assert y.P.step_count == 8
        assert torch.equal(_bits(x.P.flat), _bits(y.P.flat)) and torch.equal(_bits(x.P.m), _bits(y.P.m)) and torch.equal(_bits(x.P.v), _bits(y.P.v))
    assert not torch.equal(m1.generator.P.flat, m2.generator.P.flat)


def test_learning_rate_summary(sg, tmp_path):
    """With --lr_decay the sink gets 'Learning Rate' once per epoch, after 'Discriminator Loss', holding scheduled_lr of the
    generator's optimizer at the epoch's last step; without it the tag never appears and the tag sequence is the one
    tests/test_gpu_next_rows.py::test_epoch_end_test_pass_scores_and_summaries pins."""
    from sggan_amd.main import parse_args, synthetic_batches, synthetic_test_samples
    from sggan_amd.utils import SummarySink
    K = sg.kernels
    base = ["--img_height", "128", "--img_width", "128", "--ngf", "8", "--ndf", "8", "--batch_size", "1", "--steps_per_epoch", "2",
            "--dtype", "f32"]
    per_epoch = ["Overall Accuracy", "Mean Accuracy", "Frequency Weighted Accuracy", "Mean IoU", "Segmentation Epoch 0",
                 "Generator Loss", "Discriminator Loss"]
    def run(extra, name):
        a = parse_args(base + extra + ["--checkpoint_dir", str(tmp_path / name), "--test_dir", str(tmp_path / name / "test")])
        a.n_blocks = 2
        m = sg.sggan(a)
        sink = SummarySink()
        m.train(a, synthetic_batches(m, a), log=lambda *s: None, test_samples=synthetic_test_samples(a, count=1), sink=sink)
        return m, sink
    m, sink = run(["--epoch", "3", "--epoch_step", "1", "--lr_decay"], "a")
    tags = [r["tag"] for r in sink.records]
    assert len(tags) == 24
    for ep in range(3):
        want = list(per_epoch) + ["Learning Rate"]
        want[4] = "Segmentation Epoch %d" % ep
        assert tags[8 * ep:8 * ep + 8] == want, ep
    got = [(r["step"], r["value"]) for r in sink.records if r["tag"] == "Learning Rate"]
    assert got == [(ep, float(K.scheduled_lr(1e-3, 2 * ep + 1, 2, 1, 3))) for ep in range(3)]
    assert [v for _, v in got] == [float(np.float32(1e-3)), float(np.float32(1e-3)), float(np.float32(float(np.float32(1e-3)) / 2))]
    m, sink = run(["--epoch", "2"], "b")
    tags = [r["tag"] for r in sink.records]
    assert "Learning Rate" not in tags
    assert tags[:7] == per_epoch and tags[7:11] == per_epoch[:4] and len(tags) == 14
    assert tags[11:] == ["Segmentation Epoch 1", "Generator Loss", "Discriminator Loss"]
