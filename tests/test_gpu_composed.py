"""Train steps with EVERY option on at once against tests/composed_oracle.py: the seams between --dropout, --d_norm
spectral, --diffaug, --ssim_lambda, --ema_decay, --lr_decay, --clip_grad_norm and --skip_nonfinite in model.py, which the options'
own files (one option each, at most two) do not reach.  U-Net generators, ngf = ndf = 8, 128 x 128 (the smallest size the U-Net and
the discriminator's 1 x 1 head accept), batch 2 (the global sample index of the draws and the 2N / 4N stacked passes matter).
Bounds are the single-option files' own: losses 2e-5, every gradient tensor 2e-4 in relative L2 and worst entry over largest
(tests/test_gpu_spectral.py, tests/test_gpu_step.py), u within U_BOUND, the update at tests/test_gpu_grad_guard.py's 2e-6 and
bitwise against the plain launch, the average at tests/test_gpu_ema.py's 3 k 2^-24 max_abs."""
import random

import numpy as np
import pytest
import torch

from tests import composed_oracle as CO
from tests import ema_oracle as E
from tests import spectral_oracle as S
from tests import unet_cycle_oracle as UC
from tests import unet_oracle as UO
from tests.kink_helpers import discriminator_branches
from tests.test_gpu_spectral import U_BOUND, _kinked, _u_of, _worst
from tests.test_gpu_step import _rand_inputs

pytestmark = pytest.mark.gpu

N, H, W, C8 = 2, 128, 128, 64           # C8: the channels of d1..d3 (8 * ngf)
SCHED = (1, 1, 4)                       # rates lr, lr * 3/3, lr * 2/3, lr * 1/3: the third step's is the first to differ
U32 = 2.0 ** -24
OPTIONS = dict(d_norm="spectral", ssim_lambda=CO.SSIM_LAMBDA, ema_decay=0.999, lr_decay=True, skip_nonfinite=True)
ALL = dict(OPTIONS, use_resnet=False, ngf=8, ndf=8, dropout=CO.RATE, diffaug="color,cutout")
RESNET = dict(OPTIONS, ngf=8, ndf=8, n_blocks=1)


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


# ---- building blocks -------------------------------------------------------------------------------------------------------------
def _build(sg, clip, **kw):
    m = sg.sggan(sg.default_args(clip_grad_norm=clip, **kw))
    m.set_lr_schedule(*SCHED)
    return m


def _model(sg, prepare, **kw):
    """The model with clip_grad_norm at a quarter of the smallest gradient norm a probe step measures (the same model without a
    bound, prepared the same way), so that every network's update is clipped."""
    kw = {k: (random.Random(5) if k == "pool_rng" else v) for k, v in kw.items()}
    probe = _build(sg, 1e30, **dict(kw, graph=False, keep_tapes=False))
    prepare(probe, 0)
    probe.train_step()
    norms = {k: st["norm"] for k, st in probe.grad_stats().items()}
    assert all(0.0 < v < float("inf") for v in norms.values()), norms
    del probe
    kw = {k: (random.Random(5) if k == "pool_rng" else v) for k, v in kw.items()}
    return _build(sg, 0.25 * min(norms.values()), **kw)


def _all_clipped(m, applied=None):
    st = m.grad_stats()
    print("guard records:", {k: (round(v["norm"], 4), round(v["clip"], 4), v["skipped"], v["applied"]) for k, v in st.items()})
    assert all(v["clip"] < 1.0 for v in st.values()), st
    if applied is not None:
        assert all((v["skipped"], v["applied"]) == applied for v in st.values()), st


def _nets(m):
    return {"Gab": m.generator, "Gba": m.generator_BA, "Da": m.discriminator, "Db": m.discriminator_B} if m.cycle else \
           {"Gab": m.generator, "Da": m.discriminator}


def _load(m, P):
    for n, net in _nets(m).items():
        net.P.load(P[n])


def _export(net, buf=None):
    return {k: v.astype(np.float64) for k, v in net.P.export(buf).items()}


def _zero_pattern(xc, masks, what):
    for l in range(3):
        assert np.array_equal(xc[l].float().cpu().numpy() != 0, masks[l] != 0), f"{what}: d{l + 1}'s recorded pre-norm tensor"


def _table(m):
    return m.diffaug_params.cpu().numpy().view(np.uint32)


def _compare(step, what, got_losses, exp_losses, nets, grads, u_pairs):
    for g, e in zip(got_losses, exp_losses):
        assert abs(g - e) < 2e-5 * abs(e), (what, step, got_losses, exp_losses)
    for net, exp in u_pairs:
        U1 = _u_of(net)
        assert all(np.abs(U1[n] - exp[n]).max() <= U_BOUND for n in S.LAYERS), (what, step)
    w = {(n, k): v for n, net in nets.items() for k, v in _worst(net.P.export(net.P.grad), grads[n]).items()}
    print(f"{what}, step {step + 1}: worst", [(k, "%.1e" % a, "%.1e" % b) for k, (a, b) in sorted(w.items(), key=lambda kv: -max(kv[1]))[:4]])
    for n in nets:
        if n[0] == "D":
            assert sum(k[0] == n for k in w) == 16, n                                   # every tensor, the biases included
        else:
            assert all((n, b) in w for b in ("d1_b", "d2_b", "d3_b")) and sum(k[0] == n for k in w) == 62 - 12, n
    for n, net in nets.items():                 # (a bias in front of an unmasked instance norm: no gradient)
        got = net.P.export(net.P.grad)
        assert all(np.abs(got[k]).max() < 1e-6 for k in grads[n] if (n, k) not in w), n
    bad = {k: v for k, v in w.items() if not (v[0] < 2e-4 and v[1] < 2e-4)}
    assert not bad, (what, step, bad)


# ---- a. the reference step ---------------------------------------------------------------------------------------------------------
def _reference_oracle(m, PG, PD, U, tG, tD, real, seg, mask):
    """The composed oracle of the step ``m`` has just taken from (PG, PD, U) at the counters (tG, tD), kink-aware; checks the
    recorded zero patterns and the drawn table on the way."""
    G, D, t = m.generator, m.discriminator, m.tapes
    masks = CO.generator_masks(tG, G.seed, 0, N, H, W, C8)
    _zero_pattern([t["G"][8 + l][2] for l in range(3)], masks, "G")
    rows = CO.reference_rows(tD, N, H, W, seed=m._diffaug_seed)
    assert np.array_equal(_table(m), rows.view(np.uint32))
    br = UO.unet_branches(G, t["G"]) + discriminator_branches(D, t["D_real"]) + discriminator_branches(D, t["D_fake"])
    return _kinked(br, lambda: CO.reference_step(PG, PD, U, real, seg, mask, masks=masks, rows=rows, ssim_lambda=m.ssim_lambda,
                                                 data_range=m.ssim_data_range))


def _reference_case(sg, d_quad, **kw):
    rng = np.random.default_rng(CO.REFERENCE_CASE_SEED)
    P = CO.case_params(rng, False)
    inputs = [CO.case_inputs(rng) for _ in range(3)]

    def prepare(m, step):
        if step == 0:
            _load(m, P)
        m.real_A, m.seg_A, m.mask_A = inputs[step]
    return _model(sg, prepare, dtype="f32", d_quad=d_quad, **dict(ALL, **kw)), prepare, inputs


@pytest.mark.parametrize("d_quad", [False, True], ids=["two_passes", "d_quad"])
def test_reference_step_two_steps_match_the_composed_oracle(sg, d_quad):
    m, prepare, inputs = _reference_case(sg, d_quad, keep_tapes=True)
    G, D = m.generator, m.discriminator
    for step in range(2):
        prepare(m, step)
        PG, PD, U, tG, tD = _export(G), _export(D), _u_of(D), G.P.step_count, D.P.step_count
        assert (tG, tD) == (step, step)
        m.train_step()
        r = _reference_oracle(m, PG, PD, U, tG, tD, *inputs[step])
        _compare(step, f"reference [d_quad={d_quad}]", m.losses(), (r["gen_loss"], r["disc_loss"]), {"Gab": G, "Da": D},
                 {"Gab": r["gG"], "Da": r["gD"]}, [(D, r["U"])])
        _all_clipped(m, (0, step + 1))


# ---- b. the cycle step -------------------------------------------------------------------------------------------------------------
def _cycle_tape_masks(twin, masks, n=N):
    """G_first = (G_AB; G_BA) over the real batches: application 0; G_second = (G_BA; G_AB) over the fakes: application 1."""
    for key, app, order in (("G_first", 0, ("Gab", "Gba")), ("G_second", 1, ("Gba", "Gab"))):
        for h, name in enumerate(order):
            _zero_pattern([twin.tapes[key][8 + l][2][h * n:(h + 1) * n] for l in range(3)], masks[(name, app)], (key, name))


@pytest.mark.parametrize("cfg", [(True, True), (True, False), (False, True)], ids=["paired-d_quad", "paired-two_passes", "unpaired"])
def test_cycle_step_two_steps_match_the_composed_oracle(sg, cfg):
    paired, d_quad = cfg
    rng = np.random.default_rng(CO.CYCLE_CASE_SEED)
    P = CO.case_params(rng, True)
    inputs = [CO.case_inputs(rng) + CO.case_inputs(rng) for _ in range(2)]

    def prepare(m, step):
        if step == 0:
            _load(m, P)
        m.real_A, m.seg_A, m.mask_A, m.real_B, m.seg_B, m.mask_B = inputs[step]
    kw = dict(ALL, dtype="f32", cycle=True)
    m = _model(sg, prepare, keep_tapes=paired, d_quad=d_quad, paired=paired, **kw)
    nets = _nets(m)
    # the one-network-at-a-time step keeps no forward records: the kink decisions and the recorded zero patterns are read from a
    # lockstep twin that takes the same step from the same parameters, u and counters (tests/test_gpu_spectral.py's device)
    twin = m if paired else _build(sg, m.clip_grad_norm, keep_tapes=True, d_quad=False, paired=True, **kw)
    for step in range(2):
        prepare(m, step)
        Pn = {n: _export(net) for n, net in nets.items()}
        Ua, Ub = _u_of(nets["Da"]), _u_of(nets["Db"])
        t = {n: net.P.step_count for n, net in nets.items()}
        assert set(t.values()) == {step}
        if twin is not m:
            for net, tn in zip(nets.values(), _nets(twin).values()):
                tn.P.load(net.P.export())
                tn.P.step_count = net.P.step_count
                if tn.spectral_state() is not None:
                    tn.set_spectral_state(net.spectral_state())
            twin.real_A, twin.seg_A, twin.mask_A, twin.real_B, twin.seg_B, twin.mask_B = inputs[step]
            twin.train_step()
        m.train_step()
        rA, sA, mA, rB, sB, mB = inputs[step]
        masks = CO.cycle_masks(t["Gab"], t["Gba"], N, H, W, C8, seed=m.generator.seed)
        assert m.generator_BA.seed == m.generator.seed + 2
        _cycle_tape_masks(twin, masks)
        rows = CO.cycle_rows(t["Da"], t["Db"], N, H, W, seed=m._diffaug_seed)
        assert np.array_equal(_table(m), rows.view(np.uint32))
        sp = S.SignPolicy(1e-4, {k: getattr(m, k).numpy().astype(np.float64) for k in ("fake_A", "fake_B", "cyc_A", "cyc_B")})
        r = _kinked(UC.unet_cycle_step_branches(twin),
                    lambda: CO.cycle_step(Pn["Gab"], Pn["Gba"], Pn["Da"], Pn["Db"], Ua, Ub, rA, rB, sA, sB, mA, mB, masks=masks, rows=rows,
                                          ssim_lambda=m.ssim_lambda, data_range=m.ssim_data_range, signs=sp))
        print(f"signs: {sp.ambiguous} of {sp.elements} within 1e-4 of zero, {sp.overridden} taken the other way by the kernels")
        assert sp.disagree_outside == 0 and sp.ambiguous < 1e-3 * sp.elements
        _compare(step, f"cycle {cfg}", m.losses(), (r["g_loss"], r["d_loss"]), nets, r["grads"], [(nets["Da"], r["Ua"]), (nets["Db"], r["Ub"])])
        _all_clipped(m, (0, step + 1))


# ---- c. the update chain -----------------------------------------------------------------------------------------------------------
def _optimizers(m):
    return [m.g_optim, m.d_optim] + ([m.g_optim_BA, m.d_optim_B] if m.cycle else [])


def _feed(m, step, seed=600):
    m.real_A, m.seg_A, m.mask_A = _rand_inputs(N, H, W, m.discriminator, seed + 2 * step)
    if m.cycle:
        m.real_B, m.seg_B, m.mask_B = _rand_inputs(N, H, W, m.discriminator, seed + 1 + 2 * step)


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
def test_update_chain_spectral_transform_norm_clip_rate_average(sg, cycle):
    """Three steps (the third is the first whose scheduled rate differs from the base rate).  From each network's state before the
    step and the gradient buffer after it: the guard's record is the norm of that buffer -- for a discriminator the TRANSFORMED
    gradient, orthogonal to every kernel -- and the clip factor composed_oracle.network_update derives from it; theta, m, v are
    the plain scheduled launch at that factor bit for bit and the float64 chain at 2e-6; the generators' average is
    ema_oracle.ema_step of the new parameters at the new step count."""
    K = sg.kernels
    m = _model(sg, _feed, dtype="f32", cycle=cycle, **ALL)
    f = np.float32
    for step in range(3):
        _feed(m, step)
        before = [(o.net.P.flat.clone(), o.net.P.m.clone(), o.net.P.v.clone(), o.net.P._adam_state.clone(),
                   None if o.net.P.ema is None else o.net.P.ema.clone()) for o in _optimizers(m)]
        kernels = [None if o.net.spectral_state() is None else {n: o.net.P.p(n + "_w").double().clone() for n in S.LAYERS} for o in _optimizers(m)]
        m.train_step()
        for name, opt, (th0, m0, v0, st0, ema0), Wk in zip(m._net_names(), _optimizers(m), before, kernels):
            P = opt.net.P
            it0 = int(st0[0].item())
            assert it0 == step and opt.clip_norm == m.clip_grad_norm and (opt.ema_decay is not None) == (name[0] == "G")
            host = lambda t: {"flat": t.double().cpu().numpy()}
            th, m1, v1, it, ema, info = CO.network_update(host(th0), host(P.grad), host(m0), host(v0), it0, None if ema0 is None else host(ema0),
                                                          lr=opt.learning_rate, beta1=opt.beta_1, beta2=opt.beta_2, eps=opt.epsilon,
                                                          max_norm=opt.clip_norm, sched=SCHED, ema_decay=opt.ema_decay)
            norm, clip, skipped, applied = P._guard.tolist()
            print(f"step {step + 1} {name}: norm {norm:.6g} clip {clip:.6g} rate {info['lr']:.6g}")
            assert (skipped, applied, it, P.step_count) == (0.0, step + 1.0, step + 1, step + 1) and not info["skip"]
            assert abs(norm - info["norm"]) <= 1e-12 * norm and clip == info["clip"] < 1.0
            # (the rate the chain states decays at the third step only; that the DEVICE applied it is held by the 2e-6 bound and
            # the bitwise replay of the plain scheduled launch below, not by a record: the kernels keep none)
            assert (info["lr"] < float(f(opt.learning_rate))) == (step == 2)
            if Wk is not None:                  # the measured buffer is the transformed one: no component along any kernel
                for n in S.LAYERS:
                    g = P.g(n + "_w").double()
                    assert float(g.norm()) > 0 and abs(float((g * Wk[n]).sum())) <= 1e-5 * float(g.norm() * Wk[n].norm()), (name, n)
            for what, dev, exp in (("theta", P.flat, th), ("m", P.m, m1), ("v", P.v, v1)):
                assert np.abs(dev.cpu().numpy() - exp["flat"]).max() < 2e-6, (step, name, what)
            # ... and bit for bit the plain scheduled launch at the clipped scale and the rate of the counter before the update
            K.adam_sched(th0, P.grad, m0, v0, st0, m._lr_sched, opt.learning_rate, opt.beta_1, opt.beta_2, opt.epsilon, float(f(1.0) * f(clip)))
            assert torch.equal(th0, P.flat) and torch.equal(m0, P.m) and torch.equal(v0, P.v) and int(st0[0].item()) == step + 1, (step, name)
            if ema0 is not None:
                got = P.ema.cpu().numpy().astype(np.float64)
                want = E.ema_step(ema0.cpu().numpy(), P.flat.cpu().numpy(), opt.ema_decay, step + 1)
                max_abs = max(float(ema0.abs().max()), float(P.flat.abs().max()), float(np.abs(want).max()))
                assert np.abs(got - want).max() <= 3 * U32 * max_abs, (step, name)
                assert np.abs(got - ema["flat"]).max() <= 3 * U32 * max_abs + 2e-6, (step, name)
                assert P._ema_state.cpu().numpy().tolist() == list(E.decay_f32(opt.ema_decay, step + 1))
                assert not np.array_equal(got, P.flat.cpu().numpy().astype(np.float64))


# ---- d. bitwise invariants ---------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _state(m):
    """Everything a step leaves behind, as bit patterns (a skipped step's losses and gradients are NaN)."""
    out = [t for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.iterations, n.P.grad, n.P._guard)] + [m._loss]
    out += [n.spectral_state() for n in m.networks() if n.spectral_state() is not None]
    out += [t for n in m._ema_nets() for t in (n.P.ema, n.P._ema_state)]
    out += [m.fake_A.tensor()] + ([m.diffaug_params] if m.diffaug else [])
    return [_bits(t).clone() for t in out]


def _same(a, b, what=""):
    assert len(a) == len(b)
    for step, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for i, (p, q) in enumerate(zip(x, y)):
            assert torch.equal(p, q), (what, step, i)


def _run(m, steps, first=0):
    out = []
    for step in range(first, first + steps):
        _feed(m, step)
        m.train_step()
        out.append(_state(m))
    return out


def _finite(m):
    return all(np.isfinite(v) for v in m.losses()) and all(bool(torch.isfinite(t).all()) for n in m.networks() for t in (n.P.flat, n.P.grad, n.P.m, n.P.v))


def _adopt_draw_keys(m, run):
    """The keys of the random draws are the run's --seed (the augmentation's rows, DESIGN.md 20: "key (seed, 0) -- the model's
    seed"; the dropout masks, DESIGN.md 26: "the seed is the network's own") -- a flag of the run like the dropout rate, not state
    a checkpoint carries.  A model built with another seed, so that nothing it holds after load_state_dict can come from its own
    initialisation, is handed the run's keys here."""
    m._diffaug_seed = run._diffaug_seed
    for a, b in zip(m.networks(), run.networks()):
        a.seed = b.seed


def _expected_keys(m):
    """The union of what the options' own files state: flat / m / v / t, "arch" on G (tests/test_gpu_dropout.py: the option adds
    no key), "guard" (tests/test_gpu_grad_guard.py), "ema" on the generators (tests/test_gpu_ema.py), "d_norm" and "u" on the
    discriminators (tests/test_gpu_spectral.py); --diffaug, --ssim_lambda and --lr_decay add none."""
    base = {"flat", "m", "v", "t", "guard"}
    keys = {"G": base | {"ema", "arch"}, "D": base | {"d_norm", "u"}}
    if m.cycle:
        keys.update({"G_BA": base | {"ema"}, "D_B": base | {"d_norm", "u"}})
    return keys


def _invariants(sg, tmp_path, kw, resume=True):
    """(d): three replayed steps == three eager steps; 2 steps + save / load into a fresh model with another seed + 2 steps == 4
    steps; the state_dict's keys; bf16: everything finite."""
    eager = _model(sg, _feed, graph=False, **kw)
    clip = eager.clip_grad_norm
    whole = _run(eager, 4)
    _all_clipped(eager, (0, 4))
    assert _finite(eager)
    graph = _build(sg, clip, graph=True, **{k: (random.Random(5) if k == "pool_rng" else v) for k, v in kw.items()})
    replayed = _run(graph, 3)
    assert graph._program is not None
    _same(whole[:3], replayed, "replay")
    assert {k: set(v) for k, v in eager.state_dict().items()} == _expected_keys(eager)
    assert not torch.equal(whole[0][0], whole[1][0])
    if not resume:
        return
    m1 = _build(sg, clip, **kw)
    _same(whole[:2], _run(m1, 2), "second run")
    m1.save(str(tmp_path), 1)
    m2 = _build(sg, clip, seed=123, **kw)
    _feed(m2, 9)
    m2.train_step()                             # (every piece of state is somebody else's before the load)
    assert m2.load(str(tmp_path))
    _adopt_draw_keys(m2, m1)
    _same(whole[2:], _run(m2, 2, first=2), "resume")


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_replay_resume_and_state_keys_with_every_option(sg, tmp_path, dtype, cycle):
    _invariants(sg, tmp_path, dict(ALL, dtype=dtype, cycle=cycle))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paired_and_unpaired_cycle_steps_agree_with_every_option(sg, dtype):
    """d_quad off, one step: losses, the four images, the drawn table and u, and theta, m, v and the gradient buffer of all four
    networks and the generators' averages, bit for bit -- what tests/test_gpu_dropout.py holds bitwise at this geometry (U-Net,
    ngf = ndf = 8, 128 x 128, batch 2) in f32 with dropout alone.  tests/test_gpu_unet_cycle.py's 1e-5 rule for buffers behind a
    weight-gradient launch that two networks share is written for ngf 64; at this width the bf16 step is equal bit for bit as
    well, and is held to that.  The step keeps no data gradient once it returns; every one of them feeds a parameter gradient compared
    here (the first layers' weight gradients are taken from the joined image gradients)."""
    out, clip = [], None
    for paired in (False, True):
        kw = dict(ALL, dtype=dtype, cycle=True, paired=paired, d_quad=False)
        m = _model(sg, _feed, **kw) if clip is None else _build(sg, clip, **kw)
        clip = m.clip_grad_norm
        _feed(m, 0)
        m.train_step()
        assert (getattr(m, "_pairs", None) is not None) == paired and _finite(m)
        _all_clipped(m, (0, 1))
        exact = [m._loss, m.fake_A.tensor(), m.fake_B.tensor(), m.cyc_A.tensor(), m.cyc_B.tensor(), m.diffaug_params,
                 m.discriminator.spectral_state(), m.discriminator_B.spectral_state()]
        names = ["loss", "fake_A", "fake_B", "cyc_A", "cyc_B", "table", "u_A", "u_B"]
        names += [f"{k}.{w}" for k in m._net_names() for w in ("flat", "m", "v", "grad")] + ["G.ema", "G_BA.ema"]
        bufs = exact + [t for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.grad)] + [n.P.ema for n in m._ema_nets()]
        out.append([_bits(t).clone() for t in bufs])
    differ = [name for name, a, b in zip(names, *out) if not torch.equal(a, b)]
    print("buffers that differ between the paired and the one-network-at-a-time step:", differ)
    assert len(names) == len(out[0]) == len(out[1]) and not differ, differ


# ---- e. a skipped step in the middle -------------------------------------------------------------------------------------------------
def _poison(x):
    x = np.array(x, copy=True)
    x[0, 5, 7, 1] = np.nan                      # one pixel of one sample: a value, not a fault
    return x


def _kept_bits(m):
    """Per network, what a skipped update must leave alone: theta, m, v, iterations and, for a generator, the average and its factors."""
    out = {}
    for name, n in zip(m._net_names(), m.networks()):
        ts = [n.P.flat, n.P.m, n.P.v, n.P.iterations] + ([] if n.P.ema is None else [n.P.ema, n.P._ema_state])
        out[name] = [_bits(t).clone() for t in ts]
    return out


def _check_skips(m, before, skipped, applied_before):
    """After a step: the networks in ``skipped`` (non-finite gradient) keep every bit and count one skip; the others (finite
    gradient) are updated, clipped -- the guard decides per network."""
    st, after = m.grad_stats(), _kept_bits(m)
    print("guard records:", {k: (v["norm"], round(v["clip"], 4), v["skipped"], v["applied"]) for k, v in st.items()})
    for name, n in zip(m._net_names(), m.networks()):
        finite = bool(torch.isfinite(n.P.grad).all())
        assert finite == (name not in skipped), (name, finite)
        same = [torch.equal(a, b) for a, b in zip(before[name], after[name])]
        if name in skipped:
            assert all(same), (name, same)
            assert (st[name]["skipped"], st[name]["applied"]) == (1, applied_before) and not np.isfinite(st[name]["norm"]), st[name]
        else:
            assert not any(same), (name, same)
            assert (st[name]["skipped"], st[name]["applied"]) == (0, applied_before + 1) and st[name]["clip"] < 1.0, st[name]


def _u_advanced(D, PD, U):
    U1, _, _ = S.iterate(PD, U)
    got = _u_of(D)
    assert all(np.abs(got[n] - U1[n]).max() <= U_BOUND for n in S.LAYERS)
    assert any(np.abs(got[n] - U[n]).max() > 1e-4 for n in S.LAYERS)


@pytest.mark.parametrize("poisoned", [("real_A",), ("real_A", "seg_A")], ids=["nan_in_real_A", "nan_in_real_A_and_seg_A"])
def test_skipped_step_in_the_middle_repeats_the_draws_and_advances_u(sg, poisoned):
    """Reference step, f32, d_quad.  Step 1 is normal, step 2 reads one NaN pixel, step 3 is normal.

    nan_in_real_A: the generator's gradient is non-finite and its update is skipped.  The discriminator's is NOT: ReLU is
    ``v > 0 ? v : 0`` in the kernels and in the oracle alike, so d7's ReLU (after the skip add) hands d8 zeros for the poisoned
    sample, the fake is finite and so are both losses and D's gradient -- D's update is applied, as the per-network guard is
    documented to do.  This is the drift between the counters that key the draws: step 3 takes the masks of the
    generator's unchanged counter (1, the masks of step 2 again: DESIGN.md 20, "a skipped update ... repeats the draws") and the
    rows of the discriminator's counter (2).  Step 2 itself is held to the composed oracle where it is finite: both losses, D's
    gradient and u.
    nan_in_real_A_and_seg_A: D(seg) is non-finite too and every update is skipped -- theta, m, v, iterations, the average and its
    factors keep every bit and the skip is counted -- while u, advanced at the top of the step from the finite kernels, HAS moved
    (the power iteration belongs to the step, not to the update).  Step 3 repeats masks AND rows of t = 1.
    In both, step 3 matches the composed oracle evaluated with that u and those draws at (a)'s bounds, and a model replaying ONE
    recording takes the same three steps bit for bit."""
    m, prepare, inputs = _reference_case(sg, True, keep_tapes=True)
    real, seg, mask = inputs[1]
    inputs[1] = (_poison(real), _poison(seg) if "seg_A" in poisoned else seg, mask)
    G, D = m.generator, m.discriminator
    skipped = {"G", "D"} if "seg_A" in poisoned else {"G"}
    counters = ((0, 0), (1, 1), (1, 1 if "D" in skipped else 2))
    states = []
    for step in range(3):
        prepare(m, step)
        PG, PD, U, tG, tD = _export(G), _export(D), _u_of(D), G.P.step_count, D.P.step_count
        assert (tG, tD) == counters[step]
        before = _kept_bits(m)
        m.train_step()
        states.append(_state(m))
        if step == 1:
            _check_skips(m, before, skipped, 1)
            _u_advanced(D, PD, U)
            assert np.array_equal(_table(m), CO.reference_rows(1, N, H, W, seed=m._diffaug_seed).view(np.uint32))
            if "D" in skipped:
                assert not any(np.isfinite(v) for v in m.losses())
                continue
            with np.errstate(invalid="ignore"):
                r = _reference_oracle(m, PG, PD, U, tG, tD, *inputs[step])
            assert all(np.isfinite(v) for v in m.losses()) and bool(torch.isfinite(m.fake_A.tensor()).all())
            _compare(step, "reference, the poisoned step", m.losses(), (r["gen_loss"], r["disc_loss"]), {"Da": D}, {"Da": r["gD"]}, [(D, r["U"])])
            continue
        r = _reference_oracle(m, PG, PD, U, tG, tD, *inputs[step])       # (step 3: the masks of t = 1 again, on new data)
        _compare(step, "reference around a skipped step", m.losses(), (r["gen_loss"], r["disc_loss"]), {"Gab": G, "Da": D},
                 {"Gab": r["gG"], "Da": r["gD"]}, [(D, r["U"])])
        st = m.grad_stats()
        want = {"G": (1 if step == 2 else 0, 1 if step == 0 else 2), "D": (1 if step == 2 and "D" in skipped else 0, tD + 1)}
        assert all((st[k]["skipped"], st[k]["applied"]) == want[k] and st[k]["clip"] < 1.0 for k in st), st
    assert (G.P.step_count, D.P.step_count) == (2, 2 if "D" in skipped else 3)
    g = _build(sg, m.clip_grad_norm, dtype="f32", d_quad=True, graph=True, **ALL)
    replayed = []
    for step in range(3):
        prepare(g, step)
        g.train_step()
        replayed.append(_state(g))
    assert g._program is not None
    _same(states, replayed, "replay")


@pytest.mark.parametrize("form", [("bf16", False), ("f32", True)], ids=["bf16-unpaired", "f32-paired"])
@pytest.mark.parametrize("poisoned", [("real_A",), ("real_A", "real_B")], ids=["nan_in_real_A", "nan_in_real_A_and_real_B"])
def test_skipped_cycle_step_keeps_the_skipped_networks_and_replays(sg, poisoned, form):
    """The cycle step, invariants only (no float64 comparison: the reference-step test above carries that) -- one network at a
    time in bf16 (the U-Net's default sequencing, which keeps no forward records), and in lockstep in f32, where the recorded
    pre-norm tensors also show every step's masks: those of the generators' counters before the update, so step 3's are step
    2's again.  nan_in_real_A: G_AB, G_BA and D_A (which
    judges real_A) are skipped; D_B sees real_B and a fake_B that the generator's last ReLU made finite, and is updated -- the
    two discriminators' counters drift apart, and step 3 draws D_A's rows at 1 and D_B's at 2.  With a NaN in real_B as well all
    four are skipped.  Both discriminators' u advance either way; three replays of one recording equal the eager steps."""
    dtype, paired = form
    skipped = {"G", "D", "G_BA", "D_B"} if "real_B" in poisoned else {"G", "D", "G_BA"}
    runs, clip = [], None
    for graph in (False, True):
        kw = dict(ALL, dtype=dtype, cycle=True, graph=graph, paired=paired, keep_tapes=paired and not graph)
        m = _model(sg, _feed, **kw) if clip is None else _build(sg, clip, **kw)
        clip = m.clip_grad_norm
        Da, Db = m.discriminator, m.discriminator_B
        out = []
        for step in range(3):
            _feed(m, step)
            if step == 1:
                for name in poisoned:
                    setattr(m, name, torch.as_tensor(_poison(getattr(m, name).numpy())))
            before = _kept_bits(m)
            was = {k: (_export(D), _u_of(D)) for k, D in (("Da", Da), ("Db", Db))}
            ta, tb = Da.P.step_count, Db.P.step_count
            tg = (m.generator.P.step_count, m.generator_BA.P.step_count)
            assert (ta, tb) == ((0, 0), (1, 1), (1, 1 if "D_B" in skipped else 2))[step] and tg == ((0, 0), (1, 1), (1, 1))[step]
            m.train_step()
            out.append(_state(m))
            if m.keep_tapes:
                _cycle_tape_masks(m, CO.cycle_masks(*tg, N, H, W, C8, seed=m.generator.seed))
            if step == 0:
                _check_skips(m, before, set(), 0)
            if step == 1:
                _check_skips(m, before, skipped, 1)
                _u_advanced(Da, *was["Da"]); _u_advanced(Db, *was["Db"])
            assert np.array_equal(_table(m), CO.cycle_rows(ta, tb, N, H, W, seed=m._diffaug_seed).view(np.uint32)), step
        st = m.grad_stats()
        assert all((v["skipped"], v["applied"]) == ((1, 2) if k in skipped else (0, 3)) and v["clip"] < 1.0 for k, v in st.items()), st
        assert _finite(m)
        runs.append(out)
    _same(*runs, "replay")


# ---- f. the ResNet generator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["diffaug", "use_pool"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_resnet_invariants_with_every_option_it_has(sg, tmp_path, dtype, variant):
    """generator_resnet (one block; it has no dropout layers), cycle step, every other option on -- once with the augmentation,
    once with the static image pool in its place (the two exclude each other).  The invariants of (d); the pool's history of
    fakes is not checkpoint state, so the resume leg runs with the augmentation only."""
    if variant == "diffaug":
        _invariants(sg, tmp_path, dict(RESNET, dtype=dtype, cycle=True, diffaug="color,cutout"))
    else:
        _invariants(sg, tmp_path, dict(RESNET, dtype=dtype, cycle=True, use_pool=True, pool_static=True, max_size=2, pool_rng=None), resume=False)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_resnet_reference_step_invariants_with_every_option_it_has(sg, tmp_path, dtype):
    _invariants(sg, tmp_path, dict(RESNET, dtype=dtype, diffaug="color,cutout"))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_resnet_paired_and_unpaired_agree_with_every_option_it_has(sg, dtype):
    """tests/test_gpu_diffaug.py's rule for the paired ResNet step (d_quad off): losses, images, table and u bitwise; the rest equal
    or within 1e-5 of the norm."""
    out, clip = [], None
    for paired in (False, True):
        kw = dict(RESNET, dtype=dtype, cycle=True, paired=paired, d_quad=False, diffaug="color,cutout")
        m = _model(sg, _feed, **kw) if clip is None else _build(sg, clip, **kw)
        clip = m.clip_grad_norm
        _feed(m, 0)
        m.train_step()
        assert _finite(m)
        _all_clipped(m, (0, 1))
        out.append(([_bits(t).clone() for t in (m._loss, m.fake_A.tensor(), m.fake_B.tensor(), m.cyc_A.tensor(), m.cyc_B.tensor(),
                                                 m.diffaug_params, m.discriminator.spectral_state(), m.discriminator_B.spectral_state())],
                    [t.clone() for n in m.networks() for t in (n.P.flat, n.P.m, n.P.v, n.P.grad)]))
    assert all(torch.equal(a, b) for a, b in zip(out[0][0], out[1][0]))
    for i, (a, b) in enumerate(zip(out[0][1], out[1][1])):
        assert torch.equal(a, b) or float((a.double() - b.double()).norm() / b.double().norm()) < 1e-5, i
