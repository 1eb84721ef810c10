"""NumPy statement of the discriminators' differentiable augmentation, test infrastructure only:

  * Philox4x32-10 [Random123's constants] in Python integers, and the parameter rows ``sgg_diffaug_draw`` writes -- in float32
    arithmetic, operation for operation, so the device table can be compared bit for bit;
  * the transform and its adjoint in float64 (``forward`` / ``adjoint``);
  * the transform as one more op on ``oracle.sggan_oracle``'s tape and the reference train step with it in front of D
    (``train_step``), for the float64 restatement of the augmented step.
"""
import numpy as np

from oracle import sggan_oracle as O

F32, F64 = np.float32, np.float64
COLOR, CUTOUT = 1, 2
NEUTRAL = np.array([0, 1, 1, 0, 0, 0, 0, 0], F32)

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four 32-bit words, key: two -> four 32-bit words (ten rounds, the key bumped by the Weyl constants between rounds)."""
    c0, c1, c2, c3 = (int(c) & _MASK for c in ctr)
    k0, k1 = (int(k) & _MASK for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> 32) ^ c3 ^ k1) & _MASK, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def uniform(word):
    """u = (word >> 8) * 2^-24: 24 bits, exact in float32."""
    return F32(int(word) >> 8) * F32(2.0 ** -24)


def param_rows(t, seed, sample_offset, rows, stream_id, H, W, policy_bits, brightness=0.25):
    """The (rows, 8) float32 table [b, s, c, y0, x0, ch, cw, 0] of samples sample_offset .. sample_offset + rows - 1 at step t
    for draw stream ``stream_id`` = 2 * which_D + role (role 0: reals, 1: fakes): key (seed, 0), counter
    (t_lo, t_hi, g, 4 * stream_id + j), block j = 0 the colour draws, j = 1 the cutout's."""
    out = np.tile(NEUTRAL, (rows, 1))
    t = int(t) & 0xFFFFFFFFFFFFFFFF
    B = F32(brightness)
    for i in range(rows):
        g = (int(sample_offset) + i) & _MASK
        if policy_bits & COLOR:
            r = philox4x32_10((t & _MASK, t >> 32, g, 4 * stream_id), (seed, 0))
            out[i, 0] = F32(uniform(r[0]) - F32(0.5)) * B
            out[i, 1] = F32(2.0) * uniform(r[1])
            out[i, 2] = uniform(r[2]) + F32(0.5)
        if policy_bits & CUTOUT:
            r = philox4x32_10((t & _MASK, t >> 32, g, 4 * stream_id + 1), (seed, 0))
            ch, cw = H // 2, W // 2
            out[i, 3] = np.floor(F32(uniform(r[0]) * F32(H + 1 - ch % 2))) - F32(ch // 2)
            out[i, 4] = np.floor(F32(uniform(r[1]) * F32(W + 1 - cw % 2))) - F32(cw // 2)
            out[i, 5], out[i, 6] = ch, cw
    assert out.dtype == F32
    return out


def _inside(row, H, W):
    """(H, W) boolean: the pixels of the row's rectangle (cut to the image by construction)."""
    y0, x0, ch, cw = (int(v) for v in row[3:7])
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return (y >= y0) & (y < y0 + ch) & (x >= x0) & (x < x0 + cw)


def forward(x, params):
    """x (rows, H, W, C) real channels only, params (rows, 8) -> T(x), float64."""
    x = np.asarray(x, F64)
    out = np.empty_like(x)
    for n in range(x.shape[0]):
        b, s, c = (F64(v) for v in params[n, :3])
        H, W, C = x.shape[1:]
        x1 = x[n] + b
        m = x1.sum(-1, keepdims=True) / C
        x2 = x1 + (s - 1.0) * (x1 - m)
        M = b + x[n].sum() / (C * H * W)
        x3 = x2 + (c - 1.0) * (x2 - M)
        out[n] = np.where(_inside(params[n], H, W)[..., None], 0.0, x3)
    return out


def adjoint(g, params, addend=None):
    """The adjoint of ``forward`` (for fixed rows T is affine in x; this is the transpose of its linear part) applied to g,
    plus ``addend``."""
    g = np.asarray(g, F64)
    out = np.empty_like(g)
    for n in range(g.shape[0]):
        s, c = F64(params[n, 1]), F64(params[n, 2])
        H, W, C = g.shape[1:]
        g3 = np.where(_inside(params[n], H, W)[..., None], 0.0, g[n])
        Gs = g3.sum()
        g2 = c * g3
        out[n] = g2 + (s - 1.0) * (g2 - g2.mean(-1, keepdims=True)) + (1.0 - c) * Gs / (C * H * W)
    return out if addend is None else out + np.asarray(addend, F64)


def diff_augment(tape, x, params):
    """The transform as one op on the oracle's tape: x a Var (rows, H, W, C)."""
    y = O.Var(forward(x.v, params))
    tape.record(y, lambda gy: x.acc(adjoint(gy, params)))
    return y


def train_step(PG, PD, real_A, seg_A, mask_A, params, n_blocks=9, leak=0.3, eps=1e-3, l1_lambda=100.0):
    """oracle.sggan_oracle.train_step (model.py:169-200) with the augmentation in front of both discriminator passes:
    ``params`` (2N, 8), rows [0, N) for the reals (seg_A), [N, 2N) for the fakes.  The L1 term reads the fakes as they are.
    Activations are evaluated in the same order (G, D(seg), D(fake)), so a KinkPolicy of the plain step applies."""
    N = np.asarray(real_A).shape[0]
    tape = O.Tape()
    VG = {k: O.Var(v, k) for k, v in PG.items()}
    VD = {k: O.Var(v, k) for k, v in PD.items()}
    xA = O.Var(real_A)
    fake = O.generator_resnet(tape, VG, xA, n_blocks, eps)
    seg = O.Var(seg_A)
    da_real = O.discriminator(tape, VD, diff_augment(tape, seg, params[:N]), mask_A, leak, eps)
    da_fake = O.discriminator(tape, VD, diff_augment(tape, fake, params[N:]), mask_A, leak, eps)
    gan = O.bce_logits_mean(tape, da_fake, 1.0)
    l1 = O.l1_mean(tape, np.asarray(seg_A, F64), fake)
    gen_loss = O.scale_add(tape, gan, l1, l1_lambda)
    real_l = O.bce_logits_mean(tape, da_real, 1.0)
    fake_l = O.bce_logits_mean(tape, da_fake, 0.0)
    disc_loss = O.scale_add(tape, real_l, fake_l, 1.0)

    def grads(loss, wrt):
        for v in [xA, seg] + list(VG.values()) + list(VD.values()) + [o for o, _ in tape.ops]:
            v.g = None
        tape.backward([(loss, 1.0)])
        return {k: (np.zeros_like(v.v) if v.g is None else v.g.copy()) for k, v in wrt.items()}

    gG = grads(gen_loss, VG)
    gD = grads(disc_loss, VD)
    return {"fake_A": fake.v, "da_real": da_real.v, "da_fake": da_fake.v, "gen_loss": float(gen_loss.v),
            "disc_loss": float(disc_loss.v), "gG": gG, "gD": gD}
