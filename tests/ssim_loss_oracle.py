"""Float64 statement of the structural-similarity training loss (--ssim_lambda), test infrastructure only:

  * ``loss`` / ``grad`` / ``magnitude``: L = 1 - mean SSIM over the 11 x 11 Gaussian windows wholly inside the image, its gradient
    with respect to x in the closed form csrc/ssimloss.hip evaluates, and the magnitude M the summation-order slack of the GPU
    tests is scaled by -- NumPy, images (N,H,W,C) with real channels only;
  * ``loss_torch``: the same L from torch tensors, for float64 autograd to differentiate (the check of the closed form);
  * ``ssim_mean``: the term as one more op on ``oracle.sggan_oracle``'s tape, and with it ``train_step`` and ``cycle_step``: the
    reference step and the 2G+2D cycle step of that module with  lambda * (1 - mean SSIM)  beside every L1 reconstruction term,
    op for op in the same order, so a KinkPolicy of the plain steps applies.
"""
import numpy as np

from oracle import sggan_oracle as O

F64 = np.float64
TAPS, HALO = 11, 10


def window():
    """The 11 taps w_k ~ exp(-k^2 / (2 * 1.5^2)), k = -5..5, normalised to sum 1 (as sgg_ssim_loss forms them on the host)."""
    w = np.array([np.exp(-((k - 5.0) ** 2) / (2.0 * 1.5 * 1.5)) for k in range(TAPS)], F64)
    return w / w.sum()


def _filt(a):
    """G: the valid separable filter over axes 1 and 2 of (N,H,W,C); window p covers pixels p .. p + 10, tap k at pixel p + k."""
    w = window()
    H, W = a.shape[1], a.shape[2]
    h = sum(float(w[k]) * a[:, :, k:k + W - HALO] for k in range(TAPS))
    return sum(float(w[k]) * h[:, k:k + H - HALO] for k in range(TAPS))


def _adj(c):
    """G^T: pixel q collects the windows p in [q - 10, q] that exist, window p with tap q - p."""
    w = window()
    N, vh, vw, C = c.shape
    v = np.zeros((N, vh + HALO, vw, C), F64)
    for k in range(TAPS):
        v[:, k:k + vh] += w[k] * c
    out = np.zeros((N, vh + HALO, vw + HALO, C), F64)
    for k in range(TAPS):
        out[:, :, k:k + vw] += w[k] * v
    return out


def _terms(target, x, data_range):
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ux, uy = _filt(target), _filt(x)
    exx, eyy, exy = _filt(target * target), _filt(x * x), _filt(target * x)
    vx, vy, vxy = exx - ux * ux, eyy - uy * uy, exy - ux * uy
    A1, A2 = 2.0 * (ux * uy) + C1, 2.0 * vxy + C2
    B1, B2 = ux * ux + uy * uy + C1, vx + vy + C2
    return ux, uy, A1, A2, B1, B2, (A1 * A2) / (B1 * B2)


def ssim_map(target, x, data_range=1.0):
    return _terms(np.asarray(target, F64), np.asarray(x, F64), data_range)[-1]


def loss(target, x, data_range=1.0):
    """L = 1 - mean_{n,c,windows} S."""
    return 1.0 - ssim_map(target, x, data_range).mean()


def loss_torch(target, x, data_range=1.0):
    """The same expression on torch tensors (float64): what autograd differentiates."""
    return 1.0 - _terms(target, x, data_range)[-1].mean()


def coefficients(target, x, data_range=1.0):
    """Per window: alpha, beta, gamma with  dS = alpha d(uy) + beta d(exy) + gamma d(eyy / 2)  -- the three maps the kernel stores."""
    ux, uy, A1, A2, B1, B2, S = _terms(np.asarray(target, F64), np.asarray(x, F64), data_range)
    alpha = (2.0 * ux * A2 - 2.0 * ux * A1) / (B1 * B2) - S * 2.0 * uy / B1 + S * 2.0 * uy / B2
    return alpha, 2.0 * A1 / (B1 * B2), -2.0 * S / B2


def grad(target, x, data_range=1.0):
    """dL/dx[q] = -( (G^T alpha)[q] + target[q] (G^T beta)[q] + x[q] (G^T gamma)[q] ) / Nw."""
    target, x = np.asarray(target, F64), np.asarray(x, F64)
    a, b, g = coefficients(target, x, data_range)
    return -(_adj(a) + target * _adj(b) + x * _adj(g)) / a.size


def magnitude(target, x, data_range=1.0):
    """M[q] = (G^T|alpha| + |target| G^T|beta| + |x| G^T|gamma|) / Nw: the size of what is summed into dL/dx[q]."""
    target, x = np.asarray(target, F64), np.asarray(x, F64)
    a, b, g = coefficients(target, x, data_range)
    return (_adj(np.abs(a)) + np.abs(target) * _adj(np.abs(b)) + np.abs(x) * _adj(np.abs(g))) / a.size


# ---- the term on the oracle's tape, and the two steps with it ---------------------------------------------------------------
def ssim_mean(tape, a, b, data_range=1.0):
    """1 - mean SSIM(a, b.v) as a scalar Var; a is a constant array, b a Var (N,H,W,C)."""
    a = np.asarray(a, F64)
    y = O.Var(loss(a, b.v, data_range))
    g = grad(a, b.v, data_range)
    tape.record(y, lambda gy: b.acc(gy * g))
    return y


def train_step(PG, PD, real_A, seg_A, mask_A, ssim_lambda, data_range=1.0, n_blocks=9, leak=0.3, eps=1e-3, l1_lambda=100.0):
    """oracle.sggan_oracle.train_step (model.py:169-200) with  ssim_lambda * (1 - mean SSIM(seg_A, fake))  added to the
    generator's loss.  Activations are evaluated in the same order (G, D(seg), D(fake))."""
    tape = O.Tape()
    VG = {k: O.Var(v, k) for k, v in PG.items()}
    VD = {k: O.Var(v, k) for k, v in PD.items()}
    xA = O.Var(real_A)
    fake = O.generator_resnet(tape, VG, xA, n_blocks, eps)
    seg = O.Var(seg_A)
    da_real = O.discriminator(tape, VD, seg, mask_A, leak, eps)
    da_fake = O.discriminator(tape, VD, fake, mask_A, leak, eps)
    gan = O.bce_logits_mean(tape, da_fake, 1.0)
    l1 = O.l1_mean(tape, np.asarray(seg_A, F64), fake)
    gen_loss = O.scale_add(tape, gan, l1, l1_lambda)
    if ssim_lambda:
        gen_loss = O.scale_add(tape, gen_loss, ssim_mean(tape, seg_A, fake, data_range), ssim_lambda)
    real_l = O.bce_logits_mean(tape, da_real, 1.0)
    fake_l = O.bce_logits_mean(tape, da_fake, 0.0)
    disc_loss = O.scale_add(tape, real_l, fake_l, 1.0)

    def grads(loss_, wrt):
        for v in [xA, seg] + list(VG.values()) + list(VD.values()) + [o for o, _ in tape.ops]:
            v.g = None
        tape.backward([(loss_, 1.0)])
        return {k: (np.zeros_like(v.v) if v.g is None else v.g.copy()) for k, v in wrt.items()}

    gG = grads(gen_loss, VG)
    gD = grads(disc_loss, VD)
    return {"fake_A": fake.v, "da_real": da_real.v, "da_fake": da_fake.v, "gen_loss": float(gen_loss.v),
            "disc_loss": float(disc_loss.v), "gG": gG, "gD": gD}


def cycle_step(PGab, PGba, PDa, PDb, real_A, real_B, seg_A, seg_B, mask_A, mask_B, ssim_lambda, data_range=1.0, L1_lambda=10.0,
               Lg_lambda=5.0, use_lsgan=True, n_blocks=9, leak=0.3, eps=1e-3):
    """oracle.sggan_oracle.cycle_step (the taped form of oracle.torch_restatement.CycleStep: the same definition, and the one the
    kink-aware step tests evaluate) with the two extra terms  ssim_lambda * (1 - mean SSIM(real_A, cyc_A))  and
    ssim_lambda * (1 - mean SSIM(real_B, cyc_B))  in the generators' loss.  Gradients only (no Adam)."""
    tape = O.Tape()
    V = lambda P: {k: O.Var(v, k) for k, v in P.items()}
    Gab, Gba, Da, Db = V(PGab), V(PGba), V(PDa), V(PDb)
    xA, xB = O.Var(real_A), O.Var(real_B)
    fake_B = O.generator_resnet(tape, Gab, xA, n_blocks, eps)
    cyc_A = O.generator_resnet(tape, Gba, fake_B, n_blocks, eps)
    fake_A = O.generator_resnet(tape, Gba, xB, n_blocks, eps)
    cyc_B = O.generator_resnet(tape, Gab, fake_A, n_blocks, eps)
    DB_fake = O.discriminator(tape, Db, fake_B, mask_A, leak, eps)
    DA_fake = O.discriminator(tape, Da, fake_A, mask_B, leak, eps)
    DA_real = O.discriminator(tape, Da, xA, mask_A, leak, eps)
    DB_real = O.discriminator(tape, Db, xB, mask_B, leak, eps)
    crit = (lambda x, z: O.mse_const_mean(tape, x, z)) if use_lsgan else (lambda x, z: O.bce_logits_mean(tape, x, z))
    wA, wB = O.seg_edge_weight(seg_A), O.seg_edge_weight(seg_B)
    rA, rB = np.asarray(real_A, F64), np.asarray(real_B, F64)
    terms = [(1.0, crit(DA_fake, 1.0)), (1.0, crit(DB_fake, 1.0)),
             (L1_lambda, O.l1_mean(tape, rA, cyc_A)), (L1_lambda, O.l1_mean(tape, rB, cyc_B)),
             (Lg_lambda, O.gradloss(tape, fake_A, real_B, wB)), (Lg_lambda, O.gradloss(tape, fake_B, real_A, wA))]
    if ssim_lambda:
        terms += [(ssim_lambda, ssim_mean(tape, rA, cyc_A, data_range)), (ssim_lambda, ssim_mean(tape, rB, cyc_B, data_range))]
    g_loss = O.add_scalars(tape, terms)
    d_loss = O.add_scalars(tape, [(0.5, crit(DA_real, 1.0)), (0.5, crit(DA_fake, 0.0)),
                                  (0.5, crit(DB_real, 1.0)), (0.5, crit(DB_fake, 0.0))])
    nets = {"Gab": Gab, "Gba": Gba, "Da": Da, "Db": Db}

    def grads(loss_, which):
        for v in [xA, xB] + [p for n in nets.values() for p in n.values()] + [o for o, _ in tape.ops]:
            v.g = None
        tape.backward([(loss_, 1.0)])
        return {n: {k: (np.zeros_like(v.v) if v.g is None else v.g.copy()) for k, v in nets[n].items()} for n in which}

    G = grads(g_loss, ("Gab", "Gba"))
    G.update(grads(d_loss, ("Da", "Db")))
    return {"fake_A": fake_A.v, "fake_B": fake_B.v, "cyc_A": cyc_A.v, "cyc_B": cyc_B.v, "g_loss": float(g_loss.v),
            "d_loss": float(d_loss.v), "grads": G}
