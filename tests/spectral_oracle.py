"""Float64 NumPy statement of the spectral-norm option (``--d_norm spectral``), written from include/sggan.h and
the option's definition, not from the kernels: the power iteration, the gradient transform, a ``spectral_scale`` op for
``oracle.sggan_oracle.Tape``, and a spectrally normalised discriminator, reference step and cycle step composed from the
oracle's own primitives (as tests/ssim_loss_oracle.py composes its term).

A layer's HWIO kernel W (R, S, C, K) is the matrix M = W.reshape(R*S*C, K); u (K,) is the persistent vector."""
import numpy as np

from oracle import sggan_oracle as O

F64 = np.float64
EPS = 1e-12
LAYERS = ("h0", "h1", "h2", "h3", "h31", "h32", "h33", "h4")


def mat(W):
    W = np.asarray(W, F64)
    return W.reshape(-1, W.shape[-1])


def power_iteration(W, u, advance=True):
    """One iteration: (u', v, sigma).  advance=False: u is returned as it came and sigma = v^T M u with it."""
    M, u = mat(W), np.asarray(u, F64)
    t = M @ u
    v = t / np.sqrt(max(float(t @ t), EPS))
    if advance:
        s = M.T @ v
        u = s / np.sqrt(max(float(s @ s), EPS))
    sigma = max(float(v @ M @ u), EPS)
    return u, v, sigma


def grad_transform(dWbar, W, u, v, inv_sigma):
    """dW for dWbar = dL / d(W * inv_sigma), with u, v constants: lambda = sum(dWbar o W) * inv_sigma,
    dW = (dWbar - lambda * v u^T) * inv_sigma.  Shaped like W."""
    G, M = mat(dWbar), mat(W)
    lam = float((G * M).sum()) * inv_sigma
    return ((G - lam * np.outer(np.asarray(v, F64), np.asarray(u, F64))) * inv_sigma).reshape(np.shape(W))


def spectral_scale(tape, w, u, v):
    """Wbar = W / sigma(W) with sigma(W) = max(v^T M u, 1e-12); u and v are constants of the differentiation."""
    u, v = np.asarray(u, F64), np.asarray(v, F64)
    sigma = max(float(v @ mat(w.v) @ u), EPS)
    y = O.Var(w.v / sigma)
    tape.record(y, lambda gy: w.acc(grad_transform(gy, w.v, u, v, 1.0 / sigma)))
    return y


def discriminator_param_shapes(df_dim=64, in_c=3, segment_class=34):
    """Kernel and bias only, all eight layers (no instance norm anywhere)."""
    return [(n, s) for n, s in O.discriminator_param_shapes(df_dim, in_c, segment_class) if n.endswith(("_w", "_b"))]


def init_u(shapes, rng):
    """A unit vector per layer, length K."""
    out = {}
    for n, s in shapes:
        if n.endswith("_w"):
            d = rng.standard_normal(s[-1])
            out[n[:-2]] = d / np.linalg.norm(d)
    return out


def iterate(PD, U, advance=True):
    """Every layer's iteration on the parameters PD (name -> array): ({layer: u'}, {layer: v}, {layer: sigma})."""
    r = {n: power_iteration(PD[n + "_w"], U[n], advance) for n in LAYERS}
    return {n: a[0] for n, a in r.items()}, {n: a[1] for n, a in r.items()}, {n: a[2] for n, a in r.items()}


def scaled_kernels(tape, VD, U, V):
    """The step's normalised kernels, one Var per layer: every application of the network shares them."""
    return {n: spectral_scale(tape, VD[n + "_w"], U[n], V[n]) for n in LAYERS}


def discriminator(tape, VD, Wbar, x, mask, leak=0.3):
    """module.py:272-318 without its instance norms, on the normalised kernels."""
    h = x
    for name, stride, pad in (("h0", 2, "SAME"), ("h1", 2, "SAME"), ("h2", 2, "SAME"), ("h3", 1, "SAME"),
                              ("h31", 2, "VALID"), ("h32", 2, "VALID"), ("h33", 1, "VALID")):
        h = O.lrelu(tape, O.conv2d(tape, h, Wbar[name], VD[name + "_b"], stride, pad), leak)
    return O.mask_reduce(tape, O.conv2d(tape, h, Wbar["h4"], VD["h4_b"], 1, "SAME"), mask)


class SignPolicy:
    """Which way a sign() of the cycle step's L1 and gradient-sensitive terms points when that is not decidable at float32
    precision -- oracle.sggan_oracle.KinkPolicy's rule for the other piecewise-linear pieces of the step.  The generated images
    are float32-accurate (~1e-5), so an argument closer to zero than ``margin`` has a sign that one correct implementation takes
    one way and another the other way, and that one +-lambda/N entry of the image gradient weighs 8 x more in a 128 x 128 step
    than in a 256 x 256 one.  Such an element follows the implementation under test -- the sign of the same argument evaluated,
    in float64, on the images it generated; everywhere else the oracle keeps its own decision and a disagreement is counted
    (``disagree_outside``: an error of the implementation)."""

    def __init__(self, margin, images=None):
        self.margin, self.images = float(margin), images or {}
        self.elements = self.ambiguous = self.overridden = self.disagree_outside = 0

    def decide(self, arg, dev_arg, where=None):
        own = np.sign(arg)
        if dev_arg is None:
            return own
        live = np.ones(arg.shape, bool) if where is None else np.broadcast_to(where, arg.shape)
        dev, amb = np.sign(dev_arg), (np.abs(arg) < self.margin) & live
        diff = (dev != own) & live
        self.elements += int(live.sum()); self.ambiguous += int(amb.sum())
        self.overridden += int((diff & amb).sum()); self.disagree_outside += int((diff & ~amb).sum())
        return np.where(amb, dev, own)


def l1_mean(tape, a, b, pol=None, b_dev=None):
    """oracle.sggan_oracle.l1_mean with its sign under a SignPolicy (b_dev: the implementation's b)."""
    if pol is None or b_dev is None:
        return O.l1_mean(tape, a, b)
    d = a - b.v
    sgn = pol.decide(d, a - np.asarray(b_dev, F64))
    y = O.Var(np.abs(d).mean())
    tape.record(y, lambda gy: b.acc(-gy * sgn / d.size))
    return y


def gradloss(tape, in_, target, weight, pol=None, in_dev=None):
    """oracle.sggan_oracle.gradloss with its four signs under a SignPolicy (in_dev: the implementation's in_); only elements
    with a non-zero weight count."""
    if pol is None or in_dev is None:
        return O.gradloss(tape, in_, target, weight)
    ax, ay = O._sobel(in_.v)
    bx, by = O._sobel(np.asarray(target, F64))
    ex, ey = O._sobel(np.asarray(in_dev, F64))
    dx, dy = np.abs(ax) - np.abs(bx), np.abs(ay) - np.abs(by)
    Cn, live = in_.v.shape[-1], weight > 0
    y = O.Var((weight * (np.abs(dx) + np.abs(dy)).sum(-1, keepdims=True) / (2 * Cn)).mean())
    sx = pol.decide(dx, np.abs(ex) - np.abs(bx), live) * pol.decide(ax, ex, live)
    sy = pol.decide(dy, np.abs(ey) - np.abs(by), live) * pol.decide(ay, ey, live)

    def vjp(gy_):
        k = gy_ * weight / (2 * Cn) / weight.size
        in_.acc(O._sobel_T(k * sx, k * sy))

    tape.record(y, vjp)
    return y


def _grads(tape, loss, leaves, wrt):
    for v in leaves + [o for o, _ in tape.ops]:
        v.g = None
    tape.backward([(loss, 1.0)])
    return {k: (np.zeros_like(v.v) if v.g is None else v.g.copy()) for k, v in wrt.items()}


def discriminator_grads(PD, U, x, mask, dlogits, leak=0.3, advance=False):
    """logits of D(x | mask) and the gradient of sum(logits o dlogits) w.r.t. every stored parameter and x."""
    U1, V, S = iterate(PD, U, advance)
    tape = O.Tape()
    VD = {k: O.Var(v, k) for k, v in PD.items()}
    xv = O.Var(x)
    out = discriminator(tape, VD, scaled_kernels(tape, VD, U1, V), xv, mask, leak)
    tape.backward([(out, np.asarray(dlogits, F64))])
    g = {k: (np.zeros_like(v.v) if v.g is None else v.g) for k, v in VD.items()}
    return {"logits": out.v, "grads": g, "dx": xv.g, "U": U1, "V": V, "sigma": S}


def train_step(PG, PD, U, real_A, seg_A, mask_A, n_blocks=9, leak=0.3, eps=1e-3, l1_lambda=100.0):
    """oracle.sggan_oracle.train_step with the spectrally normalised discriminator: one power iteration on PD first, then the
    step on W / sigma.  Activations in the same order (G, D(seg), D(fake)).  Gradients only; returns the advanced u as "U"."""
    U1, V, S = iterate(PD, U)
    tape = O.Tape()
    VG = {k: O.Var(v, k) for k, v in PG.items()}
    VD = {k: O.Var(v, k) for k, v in PD.items()}
    Wbar = scaled_kernels(tape, VD, U1, V)
    xA, seg = O.Var(real_A), O.Var(seg_A)
    fake = O.generator_resnet(tape, VG, xA, n_blocks, eps)
    da_real = discriminator(tape, VD, Wbar, seg, mask_A, leak)
    da_fake = discriminator(tape, VD, Wbar, fake, mask_A, leak)
    gan = O.bce_logits_mean(tape, da_fake, 1.0)
    l1 = O.l1_mean(tape, np.asarray(seg_A, F64), fake)
    gen_loss = O.scale_add(tape, gan, l1, l1_lambda)
    disc_loss = O.scale_add(tape, O.bce_logits_mean(tape, da_real, 1.0), O.bce_logits_mean(tape, da_fake, 0.0), 1.0)
    leaves = [xA, seg] + list(VG.values()) + list(VD.values())
    gG = _grads(tape, gen_loss, leaves, VG)
    gD = _grads(tape, disc_loss, leaves, VD)
    return {"fake_A": fake.v, "da_real": da_real.v, "da_fake": da_fake.v, "gen_loss": float(gen_loss.v),
            "disc_loss": float(disc_loss.v), "gG": gG, "gD": gD, "U": U1, "V": V, "sigma": S}


def cycle_step(PGab, PGba, PDa, PDb, Ua, Ub, real_A, real_B, seg_A, seg_B, mask_A, mask_B, L1_lambda=10.0, Lg_lambda=5.0,
               use_lsgan=True, n_blocks=9, leak=0.3, eps=1e-3, signs=None):
    """oracle.sggan_oracle.cycle_step with both discriminators spectrally normalised.  Activations in its order: G_ab(real_A),
    G_ba(fake_B), G_ba(real_B), G_ab(fake_A), D_b(fake_B), D_a(fake_A), D_a(real_A), D_b(real_B).  Gradients only.
    signs: a SignPolicy whose ``images`` holds the implementation's fake_A, fake_B, cyc_A, cyc_B."""
    dev = (lambda n: signs.images.get(n)) if signs is not None else (lambda n: None)
    Ua1, Va, Sa = iterate(PDa, Ua)
    Ub1, Vb, Sb = iterate(PDb, Ub)
    tape = O.Tape()
    V = lambda P: {k: O.Var(v, k) for k, v in P.items()}
    Gab, Gba, Da, Db = V(PGab), V(PGba), V(PDa), V(PDb)
    Wa, Wb = scaled_kernels(tape, Da, Ua1, Va), scaled_kernels(tape, Db, Ub1, Vb)
    xA, xB = O.Var(real_A), O.Var(real_B)
    fake_B = O.generator_resnet(tape, Gab, xA, n_blocks, eps)
    cyc_A = O.generator_resnet(tape, Gba, fake_B, n_blocks, eps)
    fake_A = O.generator_resnet(tape, Gba, xB, n_blocks, eps)
    cyc_B = O.generator_resnet(tape, Gab, fake_A, n_blocks, eps)
    DB_fake = discriminator(tape, Db, Wb, fake_B, mask_A, leak)
    DA_fake = discriminator(tape, Da, Wa, fake_A, mask_B, leak)
    DA_real = discriminator(tape, Da, Wa, xA, mask_A, leak)
    DB_real = discriminator(tape, Db, Wb, xB, mask_B, leak)
    crit = (lambda x, z: O.mse_const_mean(tape, x, z)) if use_lsgan else (lambda x, z: O.bce_logits_mean(tape, x, z))
    wA, wB = O.seg_edge_weight(seg_A), O.seg_edge_weight(seg_B)
    rA, rB = np.asarray(real_A, F64), np.asarray(real_B, F64)
    g_loss = O.add_scalars(tape, [(1.0, crit(DA_fake, 1.0)), (1.0, crit(DB_fake, 1.0)),
                                  (L1_lambda, l1_mean(tape, rA, cyc_A, signs, dev("cyc_A"))),
                                  (L1_lambda, l1_mean(tape, rB, cyc_B, signs, dev("cyc_B"))),
                                  (Lg_lambda, gradloss(tape, fake_A, real_B, wB, signs, dev("fake_A"))),
                                  (Lg_lambda, gradloss(tape, fake_B, real_A, wA, signs, dev("fake_B")))])
    d_loss = O.add_scalars(tape, [(0.5, crit(DA_real, 1.0)), (0.5, crit(DA_fake, 0.0)),
                                  (0.5, crit(DB_real, 1.0)), (0.5, crit(DB_fake, 0.0))])
    nets = {"Gab": Gab, "Gba": Gba, "Da": Da, "Db": Db}
    leaves = [xA, xB] + [p for n in nets.values() for p in n.values()]
    both = lambda a, b: {(n, k): v for n in (a, b) for k, v in nets[n].items()}
    split = lambda g, a, b: {n: {k: v for (m, k), v in g.items() if m == n} for n in (a, b)}
    G = split(_grads(tape, g_loss, leaves, both("Gab", "Gba")), "Gab", "Gba")
    G.update(split(_grads(tape, d_loss, leaves, both("Da", "Db")), "Da", "Db"))
    return {"fake_A": fake_A.v, "fake_B": fake_B.v, "cyc_A": cyc_A.v, "cyc_B": cyc_B.v, "g_loss": float(g_loss.v),
            "d_loss": float(d_loss.v), "grads": G, "Ua": Ua1, "Ub": Ub1, "sigma_a": Sa, "sigma_b": Sb}
