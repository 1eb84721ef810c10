"""Float64 statement of the train steps with EVERY option at once, test infrastructure only: the reference step and
the 2G+2D cycle step on ``oracle.sggan_oracle``'s tape, assembled from the ops the single-option oracles export --
``unet_oracle.generator_unet`` (with the decoder's dropout masks: ``dropout``, the one new tape op), ``spectral_oracle``'s power
iteration, normalised kernels, discriminator and sign-aware L1 / gradient-sensitive terms, ``diffaug_oracle.diff_augment`` and
``ssim_loss_oracle.ssim_mean`` -- and ``network_update``, the update chain of one network (spectral gradient transform ->
global norm -> clip -> scheduled rate -> Adam -> weight average).

Every option is an argument with a neutral value: ``masks=None`` (inference-mode generators), ``rows=None`` (no augmentation),
``ssim_lambda=0``, ``U=None`` (instance-norm discriminators).  Activations are evaluated in the order of the plain steps
(unet_oracle.train_step / unet_cycle_oracle.cycle_step), so their KinkPolicy branch lists apply unchanged."""
import numpy as np

from oracle import sggan_oracle as O
from tests import diffaug_oracle as DA
from tests import dropout_oracle as DO
from tests import ema_oracle as E
from tests import spectral_oracle as S
from tests import ssim_loss_oracle as SL
from tests import unet_oracle as UO

F64 = np.float64


# ---- the generators ------------------------------------------------------------------------------------------------------------
def dropout(tape, x, mask, scale):
    """y = x * mask * scale with a fixed 0 / 1 mask (N,H,W,C): Keras Dropout in training mode with the mask handed in."""
    k = np.asarray(mask, F64) * float(scale)
    y = O.Var(x.v * k)
    tape.record(y, lambda gy: x.acc(gy * k))
    return y


def generator_unet(tape, P, x, masks=None, rate=0.5, eps=1e-3, leak=UO.LEAK):
    """unet_oracle.generator_unet with ``masks`` = the three (N,H,W,C) 0 / 1 arrays of d1, d2, d3 between the transposed conv and
    the instance norm (where dropout_oracle.torch_generator_unet puts them).  None: the inference-mode network itself."""
    if masks is None:
        return UO.generator_unet(tape, P, x, eps, leak)
    s = float(DO.scale(DO.threshold(rate)))
    norm = lambda name, z: O.instance_norm(tape, z, P[name + "_g"], P[name + "_beta"], eps)
    e, h = [], x
    for i in range(1, 8):
        h = O.lrelu(tape, norm(f"e{i}", O.conv2d(tape, h, P[f"e{i}_w"], P[f"e{i}_b"], 1, "SAME")), leak)
        e.append(h)
    h = O.relu(tape, norm("e8", O.conv2d(tape, h, P["e8_w"], P["e8_b"], 1, "SAME")))
    for i in range(1, 8):
        z = O.deconv2d(tape, h, P[f"d{i}_w"], P[f"d{i}_b"], stride=1)
        if i <= 3:
            z = dropout(tape, z, masks[i - 1], s)
        h = O.add(tape, norm(f"d{i}", z), e[7 - i])
        if i in UO.RELU_AFTER_ADD:
            h = O.relu(tape, h)
    return O.tanh(tape, O.deconv2d(tape, h, P["d8_w"], P["d8_b"], stride=1))


def _generator(kind, tape, P, x, masks, rate, n_blocks, eps):
    if kind == "resnet":
        assert masks is None, "generator_resnet has no dropout layers"
        return O.generator_resnet(tape, P, x, n_blocks, eps)
    return generator_unet(tape, P, x, masks, rate, eps)


# ---- the discriminators --------------------------------------------------------------------------------------------------------
class _Disc:
    """One discriminator of a step: spectrally normalised (U given: one power iteration first, every application on the same
    W / sigma) or the instance-norm network."""

    def __init__(self, tape, PD, U, leak, eps):
        self.tape, self.leak, self.eps = tape, leak, eps
        self.vars = {k: O.Var(v, k) for k, v in PD.items()}
        self.U1 = self.V = self.sigma = self.Wbar = None
        if U is not None:
            self.U1, self.V, self.sigma = S.iterate(PD, U)
            self.Wbar = S.scaled_kernels(tape, self.vars, self.U1, self.V)

    def __call__(self, x, mask, rows=None):
        if rows is not None:
            x = DA.diff_augment(self.tape, x, rows)
        if self.Wbar is not None:
            return S.discriminator(self.tape, self.vars, self.Wbar, x, mask, self.leak)
        return O.discriminator(self.tape, self.vars, x, mask, self.leak, self.eps)

    def scaled_grads(self):
        """dL / d(W / sigma) per layer as the last backward left them (what the device's buffer holds before spectral_grad)."""
        return None if self.Wbar is None else {n: w.g.copy() for n, w in self.Wbar.items()}


def _backward(tape, loss, leaves, nets):
    """{net: {name: dloss / dparam}} for the networks ``nets`` = {net: {name: Var}}."""
    for v in leaves + [o for o, _ in tape.ops]:
        v.g = None
    tape.backward([(loss, 1.0)])
    return {n: {k: (np.zeros_like(v.v) if v.g is None else v.g.copy()) for k, v in vs.items()} for n, vs in nets.items()}


# ---- the reference step --------------------------------------------------------------------------------------------------------
def reference_step(PG, PD, U, real_A, seg_A, mask_A, *, masks=None, rows=None, ssim_lambda=0.0, data_range=1.0, rate=0.5,
                   generator="unet", n_blocks=9, leak=0.3, eps=1e-3, l1_lambda=100.0):
    """model.py:169-200 with the options: ``masks`` the generator's three dropout masks, ``rows`` the (2N, 8) augmentation table
    [reals; fakes] (sggan.diffaug_params), ``U`` the spectral discriminator's vectors before the step.  Gradients only.
    Activations in the order G, D(seg), D(fake)."""
    N = np.asarray(real_A).shape[0]
    tape = O.Tape()
    VG = {k: O.Var(v, k) for k, v in PG.items()}
    D = _Disc(tape, PD, U, leak, eps)
    xA, seg = O.Var(real_A), O.Var(seg_A)
    fake = _generator(generator, tape, VG, xA, masks, rate, n_blocks, eps)
    da_real = D(seg, mask_A, None if rows is None else rows[:N])
    da_fake = D(fake, mask_A, None if rows is None else rows[N:])
    gan = O.bce_logits_mean(tape, da_fake, 1.0)
    l1 = O.l1_mean(tape, np.asarray(seg_A, F64), fake)
    gen_loss = O.scale_add(tape, gan, l1, l1_lambda)
    if ssim_lambda:
        gen_loss = O.scale_add(tape, gen_loss, SL.ssim_mean(tape, seg_A, fake, data_range), ssim_lambda)
    disc_loss = O.scale_add(tape, O.bce_logits_mean(tape, da_real, 1.0), O.bce_logits_mean(tape, da_fake, 0.0), 1.0)
    leaves = [xA, seg] + list(VG.values()) + list(D.vars.values())
    gG = _backward(tape, gen_loss, leaves, {"G": VG})["G"]
    gD = _backward(tape, disc_loss, leaves, {"D": D.vars})["D"]
    return {"fake_A": fake.v, "da_real": da_real.v, "da_fake": da_fake.v, "gen_loss": float(gen_loss.v),
            "disc_loss": float(disc_loss.v), "gG": gG, "gD": gD, "gD_scaled": D.scaled_grads(), "U": D.U1, "V": D.V, "sigma": D.sigma}


# ---- the cycle step ------------------------------------------------------------------------------------------------------------
def cycle_step(PGab, PGba, PDa, PDb, Ua, Ub, real_A, real_B, seg_A, seg_B, mask_A, mask_B, *, masks=None, rows=None,
               ssim_lambda=0.0, data_range=1.0, signs=None, rate=0.5, generator="unet", n_blocks=9, L1_lambda=10.0, Lg_lambda=5.0,
               use_lsgan=True, leak=0.3, eps=1e-3):
    """The 2G+2D step with the options.  ``masks``: {(network, application): [d1, d2, d3]} for ("Gab", 0) over real_A, ("Gba", 1)
    over fake_B, ("Gba", 0) over real_B, ("Gab", 1) over fake_A.  ``rows``: the (4N, 8) table in sggan.diffaug_params' order
    [D_B reals; D_B fakes; D_A fakes; D_A reals].  ``signs``: a spectral_oracle.SignPolicy holding the implementation's images.
    Activations in unet_cycle_oracle.cycle_step's order.  Gradients only."""
    N = np.asarray(real_A).shape[0]
    dev = (lambda n: signs.images.get(n)) if signs is not None else (lambda n: None)
    mk = (lambda net, app: masks[(net, app)]) if masks is not None else (lambda net, app: None)
    row = (lambda k: rows[k * N:(k + 1) * N]) if rows is not None else (lambda k: None)
    tape = O.Tape()
    Gab, Gba = ({k: O.Var(v, k) for k, v in P.items()} for P in (PGab, PGba))
    Da, Db = _Disc(tape, PDa, Ua, leak, eps), _Disc(tape, PDb, Ub, leak, eps)
    xA, xB = O.Var(real_A), O.Var(real_B)
    gen = lambda P, x, key: _generator(generator, tape, P, x, mk(*key), rate, n_blocks, eps)
    fake_B = gen(Gab, xA, ("Gab", 0))
    cyc_A = gen(Gba, fake_B, ("Gba", 1))
    fake_A = gen(Gba, xB, ("Gba", 0))
    cyc_B = gen(Gab, fake_A, ("Gab", 1))
    DB_fake = Db(fake_B, mask_A, row(1))
    DA_fake = Da(fake_A, mask_B, row(2))
    DA_real = Da(xA, mask_A, row(3))
    DB_real = Db(xB, mask_B, row(0))
    crit = (lambda x, z: O.mse_const_mean(tape, x, z)) if use_lsgan else (lambda x, z: O.bce_logits_mean(tape, x, z))
    wA, wB = O.seg_edge_weight(seg_A), O.seg_edge_weight(seg_B)
    rA, rB = np.asarray(real_A, F64), np.asarray(real_B, F64)
    terms = [(1.0, crit(DA_fake, 1.0)), (1.0, crit(DB_fake, 1.0)),
             (L1_lambda, S.l1_mean(tape, rA, cyc_A, signs, dev("cyc_A"))), (L1_lambda, S.l1_mean(tape, rB, cyc_B, signs, dev("cyc_B"))),
             (Lg_lambda, S.gradloss(tape, fake_A, real_B, wB, signs, dev("fake_A"))),
             (Lg_lambda, S.gradloss(tape, fake_B, real_A, wA, signs, dev("fake_B")))]
    if ssim_lambda:
        terms += [(ssim_lambda, SL.ssim_mean(tape, rA, cyc_A, data_range)), (ssim_lambda, SL.ssim_mean(tape, rB, cyc_B, data_range))]
    g_loss = O.add_scalars(tape, terms)
    d_loss = O.add_scalars(tape, [(0.5, crit(DA_real, 1.0)), (0.5, crit(DA_fake, 0.0)),
                                  (0.5, crit(DB_real, 1.0)), (0.5, crit(DB_fake, 0.0))])
    nets = {"Gab": Gab, "Gba": Gba, "Da": Da.vars, "Db": Db.vars}
    leaves = [xA, xB] + [p for n in nets.values() for p in n.values()]
    G = _backward(tape, g_loss, leaves, {n: nets[n] for n in ("Gab", "Gba")})
    G.update(_backward(tape, d_loss, leaves, {n: nets[n] for n in ("Da", "Db")}))
    return {"fake_A": fake_A.v, "fake_B": fake_B.v, "cyc_A": cyc_A.v, "cyc_B": cyc_B.v, "g_loss": float(g_loss.v),
            "d_loss": float(d_loss.v), "grads": G, "scaled": {"Da": Da.scaled_grads(), "Db": Db.scaled_grads()},
            "Ua": Da.U1, "Ub": Db.U1, "Va": Da.V, "Vb": Db.V, "sigma_a": Da.sigma, "sigma_b": Db.sigma}


# ---- the update chain of one network -------------------------------------------------------------------------------------------
def network_update(theta, g, m, v, iterations, ema=None, *, lr, beta1=0.5, beta2=0.999, eps=1e-7, grad_scale=1.0, max_norm=0.0,
                   sched=None, ema_decay=None, spectral=None):
    """What sggan._apply_gradients does to one network, in its order: for a spectral discriminator the gradient transform first
    (``spectral`` = (W, u, v, sigma), dicts by layer name, and ``g`` then holds dL / d(W / sigma) under ``<layer>_w``), then the
    guarded update over the WHOLE network -- global norm, clip, skip, the scheduled rate (kernels.guarded_update) -- and, where
    the update is applied, the weight average at the new step count (ema_oracle.ema_step); a skipped update leaves it alone.
    theta, g, m, v (and ema): {name: array}.  Returns (theta, m, v, iterations, ema, info); info gains "g", the gradient the
    guard measured, and "lr", the applied rate."""
    from sggan_amd import kernels as K
    names = list(theta)
    g = {k: np.asarray(g[k], F64) for k in names}
    if spectral is not None:
        W, u, vv, sigma = spectral
        for n in S.LAYERS:
            g[n + "_w"] = S.grad_transform(g[n + "_w"], W[n + "_w"], u[n], vv[n], 1.0 / sigma[n])
    flat = lambda d: np.concatenate([np.asarray(d[k], F64).reshape(-1) for k in names])
    th, m1, v1, it, info = K.guarded_update(flat(theta), flat(g), flat(m), flat(v), iterations, lr, beta1, beta2, eps, grad_scale,
                                            max_norm, sched)
    info = dict(info, g=g, lr=float(np.float32(lr)) if sched is None else float(K.scheduled_lr(lr, iterations, *sched)))
    new_ema = None
    if ema is not None:
        new_ema = flat(ema) if info["skip"] or ema_decay is None else E.ema_step(flat(ema), th, ema_decay, it)

    def split(x):
        out, off = {}, 0
        for k in names:
            shape = np.shape(theta[k])
            n = int(np.prod(shape))
            out[k], off = x[off:off + n].reshape(shape), off + n
        return out
    return split(th), split(m1), split(v1), it, (None if new_ema is None else split(new_ema)), info


# ---- the fixed cases of tests/test_gpu_composed.py (their ambiguity caps are checked on the oracle alone, tests/test_composed_cpu.py)
SEED = 19                                   # sggan's default: generators 19 / 21, discriminators 20 / 22, the augmentation's draws 19
REFERENCE_CASE_SEED, CYCLE_CASE_SEED = 141, 143
RATE, POLICY, SSIM_LAMBDA = 0.5, DA.COLOR | DA.CUTOUT, 5.0


def f32(a):
    return np.asarray(a).astype(np.float32).astype(F64)


def case_params(rng, cycle, ngf=8, ndf=8, spectral=True, generator="unet", n_blocks=1):
    """{"Gab", "Da"(, "Gba", "Db")}: float32-representable parameters, the oracle's initialisation perturbed by 0.1."""
    gs = UO.unet_param_shapes(ngf, 3, 3) if generator == "unet" else O.generator_param_shapes(gf_dim=ngf, n_blocks=n_blocks)
    ds = S.discriminator_param_shapes(df_dim=ndf) if spectral else O.discriminator_param_shapes(df_dim=ndf)
    names = ("Gab", "Gba", "Da", "Db") if cycle else ("Gab", "Da")
    return {n: {k: f32(v) for k, v in O.init_params(gs if n[0] == "G" else ds, rng, 0.1).items()} for n in names}


def case_inputs(rng, N=2, H=128, W=128):
    """(real, seg, mask): a uniform image, a 32 x 32-block palette image and one class per sample (the 1 x 1 head at 128 x 128)."""
    pal = rng.integers(0, 256, (8, 3)) / 255.0
    real = f32(rng.uniform(0, 1, (N, H, W, 3)))
    seg = f32(pal[np.repeat(np.repeat(rng.integers(0, 8, (N, H // 32, W // 32)), 32, 1), 32, 2)])
    mask = np.stack([O.one_hot(i, 34) for i in rng.integers(0, 34, (N, 1, 1))]).astype(F64)
    return real, seg, mask


def generator_masks(t, seed, application, N, H, W, C, rate=RATE, sample_offset=0):
    """The three float64 0 / 1 masks of d1..d3 for one application of a generator whose step counter reads t."""
    return [DO.layer_mask(t, seed, 4 * application + l, sample_offset, N, H, W, C, rate).astype(F64) for l in range(3)]


def reference_rows(t, N, H, W, seed=SEED, policy=POLICY):
    """sggan.diffaug_params of a reference step whose discriminator's counter reads t: [reals; fakes]."""
    return np.concatenate([DA.param_rows(t, seed, 0, N, role, H, W, policy) for role in (0, 1)])


def cycle_rows(ta, tb, N, H, W, seed=SEED, policy=POLICY):
    """sggan.diffaug_params of a cycle step: [D_B reals; D_B fakes; D_A fakes; D_A reals], stream 2 * which_D + role, D_A = 0."""
    return np.concatenate([DA.param_rows(tb, seed, 0, N, 2, H, W, policy), DA.param_rows(tb, seed, 0, N, 3, H, W, policy),
                           DA.param_rows(ta, seed, 0, N, 1, H, W, policy), DA.param_rows(ta, seed, 0, N, 0, H, W, policy)])


def cycle_masks(t_ab, t_ba, N, H, W, C, seed=SEED, rate=RATE):
    """The masks of both applications of both generators (G_AB: seed, G_BA: seed + 2) at their counters."""
    return {("Gab", a): generator_masks(t_ab, seed, a, N, H, W, C, rate) for a in (0, 1)} | \
           {("Gba", a): generator_masks(t_ba, seed + 2, a, N, H, W, C, rate) for a in (0, 1)}


def sign_counts(r, real_A, real_B, seg_A, seg_B, margin=1e-4):
    """(elements, within ``margin`` of zero) over every sign() argument of a cycle step's L1 and gradient-sensitive terms,
    evaluated on the oracle's own images ``r``."""
    pol = S.SignPolicy(margin)
    tape = O.Tape()
    for real, name in ((real_A, "cyc_A"), (real_B, "cyc_B")):
        S.l1_mean(tape, np.asarray(real, F64), O.Var(r[name]), pol, r[name])
    for name, target, seg in (("fake_A", real_B, seg_B), ("fake_B", real_A, seg_A)):
        S.gradloss(tape, O.Var(r[name]), target, O.seg_edge_weight(seg), pol, r[name])
    return pol.elements, pol.ambiguous
