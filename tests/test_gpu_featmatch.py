"""The feature-matching option (``--fm_lambda``) on the GPU: sgg_feature_match bit for bit against the emulator of
tests/featmatch_oracle.py at its chunk edges, under capture; the addend routes of the discriminator's seven consuming units against
the float64 units; the reference step against the float64 step with the term; the bitwise identities of the option off and of D's
gradient; the launch counts; the command line."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import sggan_oracle as O
from tests import featmatch_oracle as FO
from tests import spectral_oracle as S
from tests import unet_oracle as UN
from tests import unit_oracle as UO
from tests import unit_spy
from tests.kink_helpers import discriminator_branches, generator_branches
from tests.test_gpu_adam_bits import hashed_f32
from tests.test_gpu_spectral import PARENT_NODES, _captured_nodes, _kinked, _u_of, _worst, spectral_off_counts
from tests.test_gpu_step import _rand_inputs
from tests.test_gpu_unit_oracle import hashed_params

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = -7.25, 64
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
# pixels of the layers of the one L = 8 call, per dtype, Cpad 8 unless stated: a single pixel (bf16: exactly one vector), one pixel
# short of / exactly at / one pixel past the 4096-vector chunk (f32 has two vectors per pixel), more than two chunks, a 16-channel
# layer with 12 real channels, C_real 4 in Cpad 8, a pair with equal elements
EDGE = {"bf16": (4095, 4096, 4097), "f32": (2047, 2048, 2049)}


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _layers(dtype):
    a, b, c = EDGE[dtype]
    return [(1, 8, 8), (a, 8, 8), (b, 8, 8), (c, 8, 8), (2 * b + 5, 8, 8), (300, 16, 12), (77, 8, 4), (130, 8, 8)]


def _operands(dtype, layers, seed):
    """[(real, fake)] float32 host arrays (P, Cpad), values representable in ``dtype``, zeros in the padded channels; the last layer
    has equal elements in its first half."""
    rng = np.random.default_rng(seed)
    q = (lambda a: FO.bf16(a)) if dtype == "bf16" else (lambda a: a)
    out = []
    for P, Cp, Cr in layers:
        live = (np.arange(Cp) < Cr).astype(np.float32)
        r, f = (q((rng.standard_normal((P, Cp)) * live).astype(np.float32)) for _ in range(2))
        out.append((r, f))
    r, f = out[-1]
    f[: max(len(f) // 2, 1)] = r[: max(len(r) // 2, 1)]
    return out


class _Call:
    """One guarded call: every gradient buffer sits between two runs of GUARD sentinel cells."""

    def __init__(self, K, dtype, layers, ops, weight, loss0=None):
        self.K, self.dtype, self.layers, self.weight, self.loss0 = K, dtype, layers, weight, loss0
        dev = lambda a: torch.from_numpy(a).to(DT[dtype]).cuda()
        self.reals, self.fakes = [dev(r) for r, _ in ops], [dev(f) for _, f in ops]
        self.bufs = [torch.full((2 * GUARD + f.numel(),), SENTINEL, dtype=DT[dtype], device="cuda") for f in self.fakes]
        self.grads = [b[GUARD:GUARD + f.numel()].view(f.shape) for b, f in zip(self.bufs, self.fakes)]
        self.loss = torch.full((1,), 0.0 if loss0 is None else loss0, dtype=torch.float32, device="cuda")
        self.term = torch.full((1,), SENTINEL, dtype=torch.float32, device="cuda")

    def run(self):
        if self.loss0 is not None:
            self.loss.fill_(self.loss0)
        self.K.feature_match(self.reals, self.fakes, [c for _, _, c in self.layers], self.loss, self.term, self.weight,
                             accumulate_loss=self.loss0 is not None, out=self.grads)
        torch.cuda.synchronize()
        return [_bits(t).clone() for t in [self.term, self.loss] + self.grads]

    def guards_intact(self):
        return all(bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()) for b in self.bufs)


def _check(K, dtype, layers, ops, weight, loss0=None):
    call = _Call(K, dtype, layers, ops, weight, loss0)
    first = call.run()
    crs = [c for _, _, c in layers]
    term, loss, grads, chunks = FO.emulate([r for r, _ in ops], [f for _, f in ops], crs, weight, dtype == "bf16", loss=loss0)
    t64, l64, _ = K.feature_match_ref([r for r, _ in ops], [f for _, f in ops], crs, weight, loss=loss0, bf16=dtype == "bf16")
    got_t, got_l = float(call.term.item()), float(call.loss.item())
    print(f"{dtype} L={len(layers)} chunks {chunks}: term {got_t!r} (emulated {float(term)!r}, float64 {float(t64)!r}), loss {got_l!r}")
    assert np.float32(got_t).view(np.uint32) == np.float32(term).view(np.uint32)
    assert np.float32(got_l).view(np.uint32) == np.float32(loss).view(np.uint32)
    assert abs(got_t - float(t64)) <= np.spacing(np.float32(abs(float(t64))))           # 1 f32 ulp of the float64 evaluation
    for i, (g, e) in enumerate(zip(call.grads, grads)):
        assert np.array_equal(g.float().cpu().numpy().view(np.uint32), e.view(np.uint32)), (dtype, i)
    assert call.guards_intact()
    second = call.run()
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and call.guards_intact()
    return call, chunks


# ---- a. the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_kernel_is_the_emulator_bit_for_bit(sg, dtype):
    K = sg.kernels
    layers = _layers(dtype)
    ops = _operands(dtype, layers, 3)
    call, chunks = _check(K, dtype, layers, ops, 10.0)                                   # L = 8, unequal layers, overwrite
    assert chunks == [1, 1, 1, 2, 3, 1, 1, 1]
    assert any((f < r).any() for r, f in ops)                                           # negative differences
    g = call.grads[6].float().cpu().numpy()                                             # C_real 4 in Cpad 8: +0 in the pad lanes
    assert not g[:, 4:].any() and not np.signbit(g[:, 4:]).any() and g[:, :4].any()
    g = call.grads[5].float().cpu().numpy()
    assert not g[:, 12:].any() and not np.signbit(g[:, 12:]).any()
    g = call.grads[7].float().cpu().numpy()                                             # equal elements: +0
    assert not g[:65].any() and not np.signbit(g[:65]).any() and g[65:].any()
    _check(K, dtype, layers, ops, 10.0, loss0=3.5)                                      # the accumulate form
    for k in (0, 1, 3, 4):                                                              # L = 1: one vector, a chunk edge, several chunks
        _check(K, dtype, layers[k:k + 1], ops[k:k + 1], 0.75)
    same = [(r, r.copy()) for r, _ in ops]                                              # identical tensors: 0 exactly, +0 everywhere
    call, _ = _check(K, dtype, layers, same, 10.0)
    assert float(call.term.item()) == 0.0 and float(call.loss.item()) == 0.0
    assert all(not bool(_bits(g).any()) for g in call.grads)


def test_fold_crosses_its_tile_edge(sg):
    """The fold takes the partials in tiles of 512: a one-chunk layer, then a layer of 512 chunks (partials 1 .. 512, across the
    edge of the first tile, its last chunk one vector long), then a layer in the second tile -- the size at which that path exists."""
    layers = [(5, 8, 8), (511 * 4096 + 1, 8, 8), (3, 8, 8)]
    ops = _operands("bf16", layers, 6)
    _, chunks = _check(sg.kernels, "bf16", layers, ops, 10.0)
    assert chunks == [1, 512, 1]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_captured_call_replays_the_eager_bits(sg, dtype):
    from sggan_amd import kernels as Kn
    from sggan_amd.graph import StepProgram
    K = sg.kernels
    layers = _layers(dtype)
    ops = _operands(dtype, layers, 4)
    call = _Call(K, dtype, layers, ops, 2.0)
    eager = call.run()
    for t in [call.term, call.loss] + call.bufs:
        t.fill_(SENTINEL)
    prog = StepProgram("cuda")
    Kn._RECORDER = prog
    try:
        prog.record(lambda: K.feature_match(call.reals, call.fakes, [c for _, _, c in layers], call.loss, call.term, 2.0, out=call.grads))
    finally:
        Kn._RECORDER = None
    assert prog.n_graphs == 1
    prog.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, _bits(t)) for a, t in zip(eager, [call.term, call.loss] + call.grads)) and call.guards_intact()


def test_autograd_function_gives_the_term_and_its_gradient(sg):
    rng = np.random.default_rng(5)
    shapes = [(2, 5, 7, 3), (2, 3, 3, 16), (1, 1, 1, 8)]
    reals = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda() for s in shapes]
    fakes = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda().requires_grad_(True) for s in shapes]
    term = sg.feature_match(fakes, reals)
    (3.0 * term).backward()
    ref = [f.detach().clone().requires_grad_(True) for f in fakes]
    want = sum((f - r).abs().mean() for f, r in zip(ref, reals)) / 3
    (3.0 * want).backward()
    assert abs(float(term) - float(want)) <= 2e-7 * float(want)
    for f, r in zip(fakes, ref):
        assert f.grad.shape == r.grad.shape and (f.grad - r.grad).abs().max() <= 2e-7 * r.grad.abs().max()
    assert all(r.grad is None for r in reals)


# ---- b. the addend routes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("image", [(128, 128), (160, 224)], ids=["128x128", "160x224"])
def test_every_consuming_unit_adds_its_feature_gradient(sg, image, dtype):
    """D (ndf 8) at 2 x H x W: one forward, one data-gradient walk with seven addends, every recorded call held to the float64 unit
    of tests/unit_oracle.py inside its derived bound -- the stride-2 SAME, stride-1 SAME and the VALID data gradients with an addend."""
    H, W = image
    D = sg.module.Discriminator(df_dim=8, dtype=DT[dtype], device="cuda", seed=None)
    D.P.load(hashed_params(D, 3000))
    D.P.zero_grad()
    x = torch.from_numpy(hashed_f32(11, 2 * H * W * 3).reshape(2, H, W, 3)).cuda()
    mh, mw = D.out_hw(H, W)
    assert (mh, mw) == ((1, 1) if image == (128, 128) else (2, 4))
    mask = torch.nn.functional.one_hot(torch.randint(0, 34, (2, mh, mw), generator=torch.Generator().manual_seed(1)), 34).float().cuda()
    with unit_spy.Spy(D, sg._abi.route_name) as spy:
        out, tape = D.forward(D.to_internal(x), mask)
        feats = D.features(tape)
        assert len(feats) == 7 and [tuple(f.shape) for f in feats] == [tuple(r[1].shape) for r in tape[1:8]]
        assert all(f.data_ptr() == r[1].data_ptr() for f, r in zip(feats, tape[1:8]))            # views of the records: no new storage
        adds = [torch.from_numpy(0.01 * hashed_f32(20 + k, f.numel()).reshape(tuple(f.shape))).to(DT[dtype]).cuda() for k, f in enumerate(feats)]
        dy = torch.from_numpy(hashed_f32(12, out.numel()).reshape(tuple(out.shape))).cuda()
        D.backward(tape, dy, want_dx=True, param_grads=False, feature_addends=adds)
    torch.cuda.synchronize()
    back = {u.name: c for kind, u, c in spy.calls if kind == "backward"}
    assert back["h0"]["addend"] is None
    for k, name in enumerate(("h1", "h2", "h3", "h31", "h32", "h33", "h4")):
        assert back[name]["addend"] is not None and np.array_equal(back[name]["addend"].a, adds[k].float().cpu().numpy()), name
    report = {}
    bad = unit_spy.failures([r for r in unit_spy.check(spy, dtype, report) if r[2] == "backward"])
    print(f"addend routes {image} {dtype}: worst ratio per stage", json.dumps({k: float(f"{v:.4g}") for k, v in sorted(report.items())}))
    assert not bad, "\n  ".join(bad[:8])
    # slices of a stacked pass, as the step takes them
    lo = D.features(tape, 0, 1)
    assert all(a.shape[0] == 1 and a.data_ptr() == f.data_ptr() for a, f in zip(lo, feats))
    assert all(a.data_ptr() == f[1:].data_ptr() for a, f in zip(D.features(tape, 1, 2), feats))


# ---- c. the reference step against float64 -----------------------------------------------------------------------------------------
def _fm_model(sg, name, d_quad, **kw):
    spec = FO.CASES[name]
    opts = dict(ngf=8, ndf=8, n_blocks=1, dtype="f32", keep_tapes=True, d_quad=d_quad, fm_lambda=FO.FM_LAMBDA, use_resnet=spec["generator"] == "resnet")
    if spec["spectral"]:
        opts.update(d_norm="spectral", ssim_lambda=spec["ssim_lambda"], clip_grad_norm=1.0, skip_nonfinite=True)
    opts.update(kw)
    return sg.sggan(sg.default_args(**opts))


class _Tap:
    """Stands in for kernels.feature_match during a step: calls through and keeps the operands and the gradients."""

    def __init__(self, K):
        self.K, self.real, self.calls = K, K.feature_match, []

    def __enter__(self):
        def fm(reals, fakes, c_reals, loss, term, weight, accumulate_loss=False, out=None):
            grads = self.real(reals, fakes, c_reals, loss, term, weight, accumulate_loss=accumulate_loss, out=out)
            host = lambda ts: [t[..., :c].double().cpu().numpy() for t, c in zip(ts, c_reals)]
            self.calls.append(dict(real=host(reals), fake=host(fakes), grads=host(grads), weight=weight, accumulate=accumulate_loss))
            return grads
        self.K.feature_match = fm
        return self

    def __exit__(self, *exc):
        self.K.feature_match = self.real
        return False


CASES = [("resnet", True), ("resnet", False), ("unet", True), ("unet", False), ("composed", True), ("resnet160", True)]


@pytest.mark.parametrize("name,d_quad", CASES, ids=[f"{n}-{'d_quad' if q else 'two_passes'}" for n, q in CASES])
def test_reference_step_matches_the_float64_step_with_the_term(sg, name, d_quad):
    """Losses and the term 1e-5, the image 1e-4, every gradient tensor of G and of D 2e-4 of its norm -- D's against the oracle
    WITHOUT the term in its loss; the stored feature gradients to f32 rounding; no sign disagreement outside the margin."""
    spec, P, _, (real, seg, mask) = FO.case(name)
    m = _fm_model(sg, name, d_quad)
    G, D = m.generator, m.discriminator
    G.P.load(P["Gab"]); D.P.load(P["Da"])
    U = _u_of(D) if spec["spectral"] else None
    m.real_A, m.seg_A, m.mask_A = real, seg, mask
    with _Tap(sg.kernels) as tap:
        m.train_step()
    assert len(tap.calls) == 1 and len(tap.calls[0]["fake"]) == 7 and tap.calls[0]["weight"] == FO.FM_LAMBDA and tap.calls[0]["accumulate"]
    dev = tap.calls[0]
    t = m.tapes
    gen_br = generator_branches(G, t["G"]) if spec["generator"] == "resnet" else UN.unet_branches(G, t["G"])
    br = gen_br + discriminator_branches(D, t["D_real"]) + discriminator_branches(D, t["D_fake"])
    sp = S.SignPolicy(FO.MARGIN)
    r = _kinked(br, lambda: FO.case_step(name, P, U, (real, seg, mask), signs=sp, dev=dev))
    gl, dl = m.losses()
    fm = float(m.fm_loss.item())
    print(f"{name} [d_quad={d_quad}]: gen {gl!r} / {r['gen_loss']!r}, disc {dl!r} / {r['disc_loss']!r}, term {fm!r} / {r['fm_loss']!r}; "
          f"signs: {sp.ambiguous} of {sp.elements} within {FO.MARGIN} of zero, {sp.overridden} taken the other way, {sp.disagree_outside} outside")
    assert abs(gl - r["gen_loss"]) < 1e-5 * abs(r["gen_loss"]) and abs(dl - r["disc_loss"]) < 1e-5 * abs(r["disc_loss"])
    assert abs(fm - r["fm_loss"]) < 1e-5 * r["fm_loss"]
    assert np.abs(m.fake_A.numpy() - r["fake_A"]).max() < 1e-4
    assert sp.disagree_outside == 0 and sp.ambiguous <= FO.CAP * sp.elements and sp.elements == sum(f.size for f in dev["fake"])
    for k, (got, exp) in enumerate(zip(dev["grads"], r["fm_grads"])):
        assert np.abs(got - exp).max() <= 1e-6 * np.abs(exp).max() + 0.0, k
    if (spec["H"], spec["W"], spec["spectral"]) == (128, 128, False):
        # the degenerate layer: h33's map is 1 x 1, in float64 the feature is beta on both sides and the difference exactly 0.  The
        # device's norm works from f32 statistics and leaves a residue of a few 1e-7 on either side, far inside the margin: those
        # 128 signs follow the device, and nothing of them reaches G (the norm backward of a 1 x 1 map returns 0)
        assert np.array_equal(r["features"]["real"][6], r["features"]["fake"][6])
        assert np.abs(dev["real"][6] - dev["fake"][6]).max() < 1e-5
    w = {**{("D", k): v for k, v in _worst(D.P.export(D.P.grad), r["gD"]).items()}, **{("G", k): v for k, v in _worst(G.P.export(G.P.grad), r["gG"]).items()}}
    print("  worst", [(k, "%.1e" % a, "%.1e" % b) for k, (a, b) in sorted(w.items(), key=lambda kv: -kv[1][0])[:4]])
    assert sum(k[0] == "G" for k in w) >= 20 and sum(k[0] == "D" for k in w) >= 2
    bad = {k: v for k, v in w.items() if not v[0] < 2e-4}
    assert not bad, bad


# ---- d. bitwise identities ---------------------------------------------------------------------------------------------------------
def _step_state(m):
    return [_bits(t).clone() for t in (m._loss, m._fake_internal, m.generator.P.grad, m.discriminator.P.grad)]


def _small(sg, **kw):
    return sg.sggan(sg.default_args(ngf=8, ndf=8, n_blocks=1, **kw))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_off_is_the_model_without_the_argument_and_d_never_sees_the_term(sg, dtype):
    args = sg.default_args(ngf=8, ndf=8, n_blocks=1, dtype=dtype)
    del args.fm_lambda                                                                  # the flag absent from the namespace
    models = {"absent": sg.sggan(args), "zero": _small(sg, dtype=dtype, fm_lambda=0.0), "on": _small(sg, dtype=dtype, fm_lambda=10.0)}
    assert models["absent"].fm_lambda == 0.0 and models["absent"].fm_loss is None and models["zero"].fm_loss is None
    inputs = _rand_inputs(2, 128, 128, models["on"].discriminator, 40)
    states = {}
    for k, m in models.items():
        m.real_A, m.seg_A, m.mask_A = inputs
        m.train_step()
        states[k] = _step_state(m)
    assert all(torch.equal(a, b) for a, b in zip(states["absent"], states["zero"]))
    on, off = states["on"], states["zero"]
    assert torch.equal(on[3], off[3]) and torch.equal(on[1], off[1])                    # D's gradient buffer and the fakes: the same bits
    assert not torch.equal(on[2], off[2]) and not torch.equal(on[0], off[0])            # G's gradient and gen_loss: moved
    assert torch.equal(on[0][1:], off[0][1:])                                           # disc_loss: the same bits
    assert float(models["on"].fm_loss.item()) > 0


def test_bf16_graph_replay_equals_eager_over_three_steps(sg):
    runs = []
    for graph in (False, True):
        m = _small(sg, dtype="bf16", fm_lambda=10.0, graph=graph)
        out = []
        for step in range(3):
            m.real_A, m.seg_A, m.mask_A = _rand_inputs(2, 128, 128, m.discriminator, 60 + step)
            m.train_step()
            out.append(_step_state(m) + [_bits(m.fm_loss).clone(), _bits(m.generator.P.flat).clone(), _bits(m.discriminator.P.flat).clone()])
        runs.append(out)
    for a, b in zip(*runs):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert np.isfinite(m.losses()).all() and float(m.fm_loss.item()) > 0


# ---- e. launches -------------------------------------------------------------------------------------------------------------------
def test_off_launches_the_parents_step_and_on_adds_two(sg):
    got = spectral_off_counts(sg)
    print("captured nodes with the option off:", got)
    assert got == PARENT_NODES
    m = _small(sg, dtype="bf16", fm_lambda=10.0)
    m.real_A, m.seg_A, m.mask_A = _rand_inputs(2, 128, 128, m.discriminator, 40)
    with _Tap(sg.kernels) as tap:
        m.train_step()
    assert len(tap.calls) == 1 and len(tap.calls[0]["fake"]) == 7
    m._stage_inputs()
    torch.cuda.synchronize()
    assert _captured_nodes(m.device, m._step_body) == PARENT_NODES["reference"] + 2


# ---- f. the command line -----------------------------------------------------------------------------------------------------------
def test_command_line_logs_the_term_and_refuses_the_cycle_step(sg, tmp_path, capsys):
    from sggan_amd.main import main
    common = ["--batch_size", "1", "--img_height", "128", "--img_width", "128", "--ngf", "8", "--ndf", "8", "--steps_per_epoch", "2", "--epoch", "1",
              "--dataset_dir", "unit", "--log_dir", str(tmp_path / "logs"), "--checkpoint_dir", str(tmp_path / "ck"), "--test_dir", str(tmp_path / "t")]
    hist = main(["--fm_lambda", "10"] + common)
    assert len(hist) == 1 and np.isfinite([hist[0]["Generator Loss"], hist[0]["Discriminator Loss"]]).all()
    text = open(os.path.join(str(tmp_path / "logs"), "train", "scalars.jsonl")).read()
    assert "Feature Matching Loss" in text
    printed = capsys.readouterr().out
    assert printed.count("fm_loss: ") == 2
    with pytest.raises(ValueError, match="no pixel-aligned real"):
        main(["--fm_lambda", "10", "--cycle"] + common)
