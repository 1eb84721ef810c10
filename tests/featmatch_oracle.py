"""Float64 statement of the feature-matching option (``--fm_lambda``), test infrastructure only, written from the
option's definition and include/sggan.h, not from the kernels: the two discriminators restated on ``oracle.sggan_oracle``'s tape WITH
their seven taps (``O.discriminator`` / ``S.discriminator`` return the logits only), the term as a tape op under
``spectral_oracle.SignPolicy``, the reference step with the term composed from ``composed_oracle``'s pieces, and ``emulate``, the
kernel's magnitudes and summation order in NumPy.

The taps are the post-activation outputs of h0 .. h33; h4's output, the logit map, is not one."""
import numpy as np

from oracle import sggan_oracle as O
from tests import composed_oracle as CO
from tests import spectral_oracle as S
from tests import ssim_loss_oracle as SL

F64 = np.float64
TAPS = ("h0", "h1", "h2", "h3", "h31", "h32", "h33")
_TAIL = (("h1", 2, "SAME"), ("h2", 2, "SAME"), ("h3", 1, "SAME"), ("h31", 2, "VALID"), ("h32", 2, "VALID"), ("h33", 1, "VALID"))


# ---- the discriminators with their taps ------------------------------------------------------------------------------------------
def discriminator(tape, P, x, mask, leak=0.3, eps=1e-3):
    """O.discriminator (module.py:272-318), op for op and in its activation order: (logits, [the seven features], the h4 map)."""
    h = O.lrelu(tape, O.conv2d(tape, x, P["h0_w"], P["h0_b"], 2, "SAME"), leak)
    feats = [h]
    for name, stride, pad in _TAIL:
        h = O.conv2d(tape, h, P[name + "_w"], P[name + "_b"], stride, pad)
        h = O.lrelu(tape, O.instance_norm(tape, h, P[name + "_g"], P[name + "_beta"], eps), leak)
        feats.append(h)
    h4 = O.conv2d(tape, h, P["h4_w"], P["h4_b"], 1, "SAME")
    return O.mask_reduce(tape, h4, mask), feats, h4


def spectral_discriminator(tape, VD, Wbar, x, mask, leak=0.3):
    """S.discriminator (no instance norm anywhere, the normalised kernels), with the taps."""
    h, feats = x, []
    for name, stride, pad in (("h0", 2, "SAME"),) + _TAIL:
        h = O.lrelu(tape, O.conv2d(tape, h, Wbar[name], VD[name + "_b"], stride, pad), leak)
        feats.append(h)
    h4 = O.conv2d(tape, h, Wbar["h4"], VD["h4_b"], 1, "SAME")
    return O.mask_reduce(tape, h4, mask), feats, h4


class _Disc(CO._Disc):
    """composed_oracle._Disc handing out the taps: (logits, features, h4 map) per application."""

    def __call__(self, x, mask):
        if self.Wbar is not None:
            return spectral_discriminator(self.tape, self.vars, self.Wbar, x, mask, self.leak)
        return discriminator(self.tape, self.vars, x, mask, self.leak, self.eps)


# ---- the term ------------------------------------------------------------------------------------------------------------------------
def feature_match(tape, reals, fakes, signs=None, dev_fakes=None, dev_reals=None, *, layer_sum=False, count_pad=None, sign0=0.0,
                  grads_out=None):
    """term = (1/L) sum_i mean |fake_i - real_i| as a tape scalar; the reals (Vars or arrays) are constants, fake_i gets
    gy * sign(fake_i - real_i) / (L * count_i).  signs: a spectral_oracle.SignPolicy -- an argument within its margin of zero takes
    the sign of the same difference on the implementation's features (dev_fakes, dev_reals; dev_reals None: the oracle's reals).
    The keywords plant errors (tests/test_featmatch_cpu.py): layer_sum -- the sum over layers instead of their mean; count_pad --
    a function C -> padded C whose count replaces count_i; sign0 -- the value of sign(0).  grads_out: a list that receives
    dterm / dfake_i per pair."""
    reals = [np.asarray(r.v if isinstance(r, O.Var) else r, F64) for r in reals]
    L = len(fakes)
    assert len(reals) == L and all(r.shape == f.v.shape for r, f in zip(reals, fakes))
    div = 1.0 if layer_sum else float(L)
    value, sgns, counts = 0.0, [], []
    for i, (r, f) in enumerate(zip(reals, fakes)):
        d = f.v - r
        count = d.size if count_pad is None else d.size // d.shape[-1] * count_pad(d.shape[-1])
        if signs is not None and dev_fakes is not None:
            dr = r if dev_reals is None else np.asarray(dev_reals[i], F64)
            sgn = signs.decide(d, np.asarray(dev_fakes[i], F64) - dr)
        else:
            sgn = np.sign(d)
        sgn = np.where(d == 0, sign0, sgn) if sign0 else sgn
        value += np.abs(d).sum() / count
        sgns.append(sgn); counts.append(count)
    y = O.Var(value / div)
    if grads_out is not None:
        grads_out.extend(sgn / (div * count) for sgn, count in zip(sgns, counts))

    def vjp(gy):
        for f, sgn, count in zip(fakes, sgns, counts):
            f.acc(gy * sgn / (div * count))

    tape.record(y, vjp)
    return y


# ---- the reference step with the term --------------------------------------------------------------------------------------------
def reference_step(PG, PD, U, real_A, seg_A, mask_A, *, fm_lambda, signs=None, dev=None, masks=None, ssim_lambda=0.0, data_range=1.0,
                   rate=0.5, generator="resnet", n_blocks=1, leak=0.3, eps=1e-3, l1_lambda=100.0, in_disc_loss=False, with_logits=False,
                   **planted):
    """composed_oracle.reference_step (no augmentation: the option refuses it) with gen_loss += fm_lambda * feature_match over the
    taps of D(seg) (constants) and D(fake).  dev = {"real": [...], "fake": [...]}: the implementation's features for ``signs``.
    Activations in the order G, D(seg), D(fake), as the plain step's.  Planted errors: in_disc_loss -- the term added to disc_loss
    as well; with_logits -- the h4 map as an eighth pair; the rest go to feature_match.  Returns composed_oracle's dict + "fm_loss",
    "fm_grads" (fm_lambda * dterm / dfeature per pair: what the kernel stores) and "features"."""
    tape = O.Tape()
    VG = {k: O.Var(v, k) for k, v in PG.items()}
    D = _Disc(tape, PD, U, leak, eps)
    xA, seg = O.Var(real_A), O.Var(seg_A)
    fake = CO._generator(generator, tape, VG, xA, masks, rate, n_blocks, eps)
    da_real, f_real, m_real = D(seg, mask_A)
    da_fake, f_fake, m_fake = D(fake, mask_A)
    gan = O.bce_logits_mean(tape, da_fake, 1.0)
    l1 = O.l1_mean(tape, np.asarray(seg_A, F64), fake)
    gen_loss = O.scale_add(tape, gan, l1, l1_lambda)
    if ssim_lambda:
        gen_loss = O.scale_add(tape, gen_loss, SL.ssim_mean(tape, seg_A, fake, data_range), ssim_lambda)
    dev = dev or {}
    extra = ([m_real], [m_fake]) if with_logits else ([], [])
    fm_grads = []
    fm = feature_match(tape, f_real + extra[0], f_fake + extra[1], signs, dev.get("fake"), dev.get("real"), grads_out=fm_grads, **planted)
    gen_loss = O.scale_add(tape, gen_loss, fm, fm_lambda)
    disc_loss = O.scale_add(tape, O.bce_logits_mean(tape, da_real, 1.0), O.bce_logits_mean(tape, da_fake, 0.0), 1.0)
    if in_disc_loss:
        # (a term in D's loss is differentiated through BOTH passes: the reals are no constants there)
        disc_loss = O.scale_add(tape, disc_loss, _two_sided(tape, f_real, f_fake), fm_lambda)
    leaves = [xA, seg] + list(VG.values()) + list(D.vars.values())
    gG = CO._backward(tape, gen_loss, leaves, {"G": VG})["G"]
    gD = CO._backward(tape, disc_loss, leaves, {"D": D.vars})["D"]
    return {"fake_A": fake.v, "da_real": da_real.v, "da_fake": da_fake.v, "gen_loss": float(gen_loss.v), "disc_loss": float(disc_loss.v),
            "fm_loss": float(fm.v), "fm_grads": [fm_lambda * g for g in fm_grads], "gG": gG, "gD": gD, "gD_scaled": D.scaled_grads(),
            "U": D.U1, "V": D.V, "sigma": D.sigma,
            "features": {"real": [f.v for f in f_real], "fake": [f.v for f in f_fake]}}


def _two_sided(tape, reals, fakes):
    """The term with gradient to both operands (the planted error only)."""
    L = len(fakes)
    y = O.Var(sum(np.abs(f.v - r.v).mean() for r, f in zip(reals, fakes)) / L)

    def vjp(gy):
        for r, f in zip(reals, fakes):
            s = np.sign(f.v - r.v) * gy / (L * f.v.size)
            f.acc(s); r.acc(-s)

    tape.record(y, vjp)
    return y


def sign_counts(features, margin=1e-4):
    """(elements, within ``margin`` of zero, exactly zero) over every sign() argument of the term on the oracle's own features."""
    d = [np.asarray(f, F64) - np.asarray(r, F64) for r, f in zip(features["real"], features["fake"])]
    return sum(x.size for x in d), sum(int((np.abs(x) < margin).sum()) for x in d), sum(int((x == 0).sum()) for x in d)


# ---- the kernel's arithmetic -----------------------------------------------------------------------------------------------------
THREADS, CHUNK, WAVE = 256, 4096, 64         # FM_THREADS, FM_CHUNK (16-byte vectors per block), the wave


def bf16(a):
    """float32 array rounded to bfloat16 (nearest even), returned as float32."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _chunk_sum(a):
    """One block's double: a (vectors, VEC) float64 of |d| (0 where masked), vectors <= CHUNK."""
    nv, vec = a.shape
    rows = -(-nv // THREADS)
    pad = np.zeros((rows * THREADS, vec), F64)
    pad[:nv] = a
    pad = pad.reshape(rows, THREADS, vec)
    s = np.zeros(THREADS, F64)
    for k in range(rows):                    # lane t: its vectors t, t + 256, ... ascending, the elements of a vector ascending
        for e in range(vec):
            s = s + pad[k, :, e]
    v = s.reshape(THREADS // WAVE, WAVE)
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):           # the butterfly: every lane adds its partner's value
        v = v + v[:, lane ^ o]
    w = v[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def emulate(reals, fakes, c_reals, weight, bf16_storage=False, loss=None):
    """sgg_feature_match on padded (..., Cpad) float32 arrays (bf16_storage: their values are bfloat16-representable and the
    gradients are rounded to bfloat16): (float32 term, float32 loss, [float32 grad_i], [the layers' chunk counts]) with every sum in
    the kernel's order -- per block lane-strided, the butterfly, the waves in order; per layer the chunks in index order; the layers
    in order -- and the magnitudes float32(weight / (L * count_i)).  loss: the scalar's old value (the accumulate form) or None."""
    f = np.float32
    vec = 8 if bf16_storage else 4
    L, w = len(fakes), float(f(weight))
    means, grads, chunks = [], [], []
    for r, x, c in zip(reals, fakes, c_reals):
        r, x = np.asarray(r, f), np.asarray(x, f)
        Cp = x.shape[-1]
        d = x.astype(F64) - r.astype(F64)
        live = np.broadcast_to(np.arange(Cp) < c, d.shape)
        a = np.where(live, np.abs(d), 0.0).reshape(-1, vec)
        count = float(d.size // Cp * c)
        n = -(-a.shape[0] // CHUNK)
        s = 0.0
        for k in range(n):
            s = s + _chunk_sum(a[k * CHUNK:(k + 1) * CHUNK])
        means.append(s / count)
        chunks.append(n)
        mag = f(w / (L * count))
        g = np.where(live, np.where(d > 0, mag, np.where(d < 0, -mag, f(0))), f(0)).astype(f)
        grads.append(bf16(g) if bf16_storage else g)
    m = means[0]
    for x in means[1:]:
        m = m + x
    m = m / float(L)
    out = f(w * m)
    return f(m), (out if loss is None else f(f(loss) + out)), grads, chunks


# ---- the fixed cases of tests/test_gpu_featmatch.py (their ambiguity caps are checked on the oracle alone, tests/test_featmatch_cpu.py)
FM_LAMBDA, MARGIN, CAP = 10.0, 1e-4, 5e-3
CASES = {"resnet": dict(generator="resnet", spectral=False, H=128, W=128),
         "unet": dict(generator="unet", spectral=False, H=128, W=128),
         "composed": dict(generator="resnet", spectral=True, H=128, W=128, ssim_lambda=CO.SSIM_LAMBDA),
         "resnet160": dict(generator="resnet", spectral=False, H=160, W=224)}


def case(name, N=2):
    """(spec, {"Gab", "Da"}, U or None, (real, seg, mask)) of a fixed case: composed_oracle's parameters and inputs at
    REFERENCE_CASE_SEED, ngf = ndf = 8, one residual block; the mask one class per cell of D's output grid."""
    spec = CASES[name]
    rng = np.random.default_rng(CO.REFERENCE_CASE_SEED)
    P = CO.case_params(rng, False, spectral=spec["spectral"], generator=spec["generator"], n_blocks=1)
    real, seg, mask = CO.case_inputs(rng, N, spec["H"], spec["W"])
    mh, mw = O.disc_out_hw(spec["H"], spec["W"])
    if (mh, mw) != (1, 1):
        mask = np.stack([O.one_hot(i, 34) for i in rng.integers(0, 34, (N, mh, mw))]).astype(F64)
    U = S.init_u(S.discriminator_param_shapes(df_dim=8), rng) if spec["spectral"] else None
    return spec, P, U, (real, seg, mask)


def case_step(name, P, U, inputs, **kw):
    spec = CASES[name]
    return reference_step(P["Gab"], P["Da"], U, *inputs, fm_lambda=FM_LAMBDA, generator=spec["generator"], n_blocks=1,
                          ssim_lambda=spec.get("ssim_lambda", 0.0), **kw)
