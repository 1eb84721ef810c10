"""Float64 statement of the resize-convolution option of generator_resnet, on ``oracle.sggan_oracle``'s tape: the
fixed 2x resampling U with its vjp, the generator with d1 / d2 replaced, the reference step and the cycle step with that
generator handed in (the loss ops are the ones ``O.train_step`` / ``O.cycle_step`` use; those two fix ``O.generator_resnet``),
and -- for the bitwise kernel tests -- emulators of the kernels' f32 tap order and single rounding.

U, NHWC, (N,H,W,C) -> (N,2H,2W,C), per axis of length n and the 2-D operator the tensor product of the two axes:
    nearest    y[2i] = y[2i+1] = x[i]
    bilinear   y[2i] = 0.25 x[max(i-1,0)] + 0.75 x[i],   y[2i+1] = 0.75 x[i] + 0.25 x[min(i+1,n-1)]        (half-pixel centres)
U^T per axis: nearest dx[i] = g[2i] + g[2i+1]; bilinear dx[i] = sum_{k=-1..2} w_k g[clamp(2i+k, 0, 2n-1)], w = (1/4, 3/4, 3/4, 1/4)
-- written here as the scatter of the forward's taps, so that the clamp form the kernel uses is checked against it.

The bound where inputs are fractional (``bound``).  The kernel forms acc = w_0 v_0, acc = acc + w_t v_t (t = 1..T-1) with every
product and every sum rounded to f32, unit roundoff u = 2^-24, then rounds once to the storage type.  The weights are exact.
Product t carries an error of at most u |w_t v_t|.  The t-th sum rounds a value of magnitude at most (1 + O(u)) sum_{s<=t} |w_s v_s|
<= (1 + O(u)) S with S = sum_t |w_t v_t|: at most u S (1 + O(u)) each, T - 1 of them.  Together at most
u S + (T - 1) u S = T u S to first order; the second-order terms are bounded by (T u)^2 S, kept as the factor (1 + T u).  The
storage rounding adds at most half an ulp of the storage type at the magnitude of the f32 result, which lies within that first
term of the exact one: half_ulp(|exact| + T u S).  T = 4 (bilinear forward), 16 (bilinear adjoint), 4 (nearest adjoint, no
products: (T - 1) u S <= T u S); the nearest forward is a copy and is compared exactly."""
import numpy as np
import torch

from oracle import sggan_oracle as O

F64 = np.float64
MODES = ("nearest", "bilinear")
TAPS = {("nearest", "bwd"): 4, ("bilinear", "fwd"): 4, ("bilinear", "bwd"): 16}


# ----------------------------------------------------------------------------- the operator, float64
def _take(x, idx, axis):
    return np.take(x, idx, axis=axis)


def _up_axis(x, axis, mode):
    n = x.shape[axis]
    if mode == "nearest":
        return np.repeat(x, 2, axis=axis)
    i = np.arange(n)
    even = 0.25 * _take(x, np.maximum(i - 1, 0), axis) + 0.75 * x
    odd = 0.75 * x + 0.25 * _take(x, np.minimum(i + 1, n - 1), axis)
    y = np.stack([even, odd], axis=axis + 1)
    return y.reshape(x.shape[:axis] + (2 * n,) + x.shape[axis + 1:])


def _up_axis_T(g, axis, mode):
    n = g.shape[axis] // 2
    ge, go = _take(g, np.arange(0, 2 * n, 2), axis), _take(g, np.arange(1, 2 * n, 2), axis)
    if mode == "nearest":
        return ge + go
    i = np.arange(n)
    dx = np.moveaxis(0.75 * (ge + go), axis, 0).copy()
    np.add.at(dx, np.maximum(i - 1, 0), 0.25 * np.moveaxis(ge, axis, 0))        # y[2i] took 0.25 x[max(i-1,0)]
    np.add.at(dx, np.minimum(i + 1, n - 1), 0.25 * np.moveaxis(go, axis, 0))    # y[2i+1] took 0.25 x[min(i+1,n-1)]
    return np.moveaxis(dx, 0, axis)


def up(x, mode):
    """U x for an NHWC array (float64)."""
    assert mode in MODES
    return _up_axis(_up_axis(np.asarray(x, F64), 1, mode), 2, mode)


def up_T(g, mode):
    """U^T g."""
    assert mode in MODES
    return _up_axis_T(_up_axis_T(np.asarray(g, F64), 2, mode), 1, mode)


def upsample2x(tape, x: O.Var, mode) -> O.Var:
    y = O.Var(up(x.v, mode))
    tape.record(y, lambda gy: x.acc(up_T(gy, mode)))
    return y


# ----------------------------------------------------------------------------- the kernels' arithmetic
def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _store(acc, bf16):
    return _bf16(acc) if bf16 else acc


def emulate_fwd(x, mode, bf16=False):
    """sgg_upsample2x_fwd on an f32 array holding storage-type values: the kernel's taps in its order, f32 products and sums,
    one rounding to the storage type.  Nearest: the gather (a copy)."""
    x = np.asarray(x, np.float32)
    N, H, W, C = x.shape
    if mode == "nearest":
        return x[:, np.arange(2 * H) >> 1][:, :, np.arange(2 * W) >> 1]
    i, j = np.arange(H), np.arange(W)
    ri = [np.maximum(i - 1, 0), i, np.minimum(i + 1, H - 1)]
    ci = [np.maximum(j - 1, 0), j, np.minimum(j + 1, W - 1)]
    y = np.empty((N, 2 * H, 2 * W, C), np.float32)
    q, t = np.float32(0.25), np.float32(0.75)
    for a in range(2):
        for b in range(2):
            wr, wc = ((q, t), (t, q))[a], ((q, t), (t, q))[b]
            tap = lambda r, c: (wr[r] * wc[c]) * x[:, ri[a + r]][:, :, ci[b + c]]         # f32 product, rounded
            acc = tap(0, 0)
            acc = acc + tap(0, 1)
            acc = acc + tap(1, 0)
            acc = acc + tap(1, 1)
            y[:, a::2, b::2] = acc
    return _store(y, bf16)


def emulate_bwd(dy, mode, bf16=False):
    """sgg_upsample2x_bwd likewise: the 2x2 block sum, or the 16 clamped taps row-major over the source offsets -1..2."""
    dy = np.asarray(dy, np.float32)
    N, H2, W2, C = dy.shape
    H, W = H2 // 2, W2 // 2
    i, j = np.arange(H), np.arange(W)
    if mode == "nearest":
        d = lambda a, b: dy[:, 2 * i + a][:, :, 2 * j + b]
        return _store(((d(0, 0) + d(0, 1)) + d(1, 0)) + d(1, 1), bf16)
    w = (np.float32(0.25), np.float32(0.75), np.float32(0.75), np.float32(0.25))
    acc = None
    for r in range(4):
        rows = np.clip(2 * i - 1 + r, 0, 2 * H - 1)
        for c in range(4):
            cols = np.clip(2 * j - 1 + c, 0, 2 * W - 1)
            p = (w[r] * w[c]) * dy[:, rows][:, :, cols]
            acc = p if acc is None else acc + p
    return _store(acc, bf16)


def half_ulp(v, bf16):
    """Half a unit in the last place of the storage type at magnitude |v| (normal range)."""
    p = 8 if bf16 else 24
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 0.5 * 2.0 ** (e - (p - 1))


def bound(x, mode, direction, bf16):
    """(exact result in float64, the per-element bound of the module docstring) for the kernel applied to x."""
    op = up if direction == "fwd" else up_T
    exact, S = op(x, mode), op(np.abs(np.asarray(x, F64)), mode)
    T, u = TAPS[(mode, direction)], 2.0 ** -24
    first = T * u * S * (1 + T * u)
    return exact, first + half_ulp(np.abs(exact) + first, bf16)


# ----------------------------------------------------------------------------- the network and the steps
class SignPolicy:
    """The kinks of the loss terms -- sign() in the L1 terms and in the gradient-sensitive terms -- handled as O.KinkPolicy handles
    the activations'.  One flipped sign moves one entry of an image gradient whose entries are all +-lambda / n: 2 / sqrt(n) of its
    norm, and the parameter gradients, incoherent sums over those entries, by as much -- 6e-3 at n = 2 * 128 * 128 * 3, measured
    2.5e-3 to 7.8e-3 on the steps where a difference lay within 1e-6 of zero.  An argument within ``margin`` of zero is undecidable at
    float32 precision: there the reference takes the sign the kernels saw, which is the sign of the same expression evaluated (in
    float64) on the images the DEVICE produced; everywhere else it keeps its own and counts a disagreement (``disagree_outside``)."""

    def __init__(self, margin=1e-4):
        self.margin, self.ambiguous, self.overridden, self.disagree_outside = float(margin), 0, 0, 0

    def sign(self, own, device):
        s, e = np.sign(own), np.sign(device)
        amb = np.abs(own) < self.margin
        self.ambiguous += int(amb.sum())
        self.overridden += int(((s != e) & amb).sum())
        self.disagree_outside += int(((s != e) & ~amb).sum())
        return np.where(amb, e, s)


def l1_mean(tape, a, b: O.Var, signs=None, device_b=None) -> O.Var:
    """O.l1_mean; with a SignPolicy, the vjp's sign(a - b) follows sign(a - device_b) inside the band."""
    d = a - b.v
    y = O.Var(np.abs(d).mean())
    s = np.sign(d) if signs is None else signs.sign(d, a - np.asarray(device_b, F64))
    tape.record(y, lambda gy: b.acc(-gy * s / d.size))
    return y


def gradloss(tape, in_: O.Var, target, weight, signs=None, device_in=None) -> O.Var:
    """O.gradloss; with a SignPolicy, sign(tf_deriv(in_)) and sign(|tf_deriv(in_)| - |tf_deriv(target)|) in the vjp follow the same
    expressions on the device's image inside the band."""
    ax, ay = O._sobel(in_.v)
    bx, by = O._sobel(np.asarray(target, F64))
    dx, dy = np.abs(ax) - np.abs(bx), np.abs(ay) - np.abs(by)
    C = in_.v.shape[-1]
    y = O.Var((weight * ((np.abs(dx) + np.abs(dy)).sum(-1, keepdims=True) / (2 * C))).mean())
    if signs is None:
        sax, say, sdx, sdy = np.sign(ax), np.sign(ay), np.sign(dx), np.sign(dy)
    else:
        ex, ey = O._sobel(np.asarray(device_in, F64))
        sax, say = signs.sign(ax, ex), signs.sign(ay, ey)
        sdx, sdy = signs.sign(dx, np.abs(ex) - np.abs(bx)), signs.sign(dy, np.abs(ey) - np.abs(by))

    def vjp(gy_):
        k = gy_ * weight / (2 * C) / weight.size
        in_.acc(O._sobel_T(k * sdx * sax, k * sdy * say))

    tape.record(y, vjp)
    return y


def generator_param_shapes(gf_dim=64, in_c=3, out_c=3, n_blocks=9):
    """O.generator_param_shapes with d1_w / d2_w in the Conv2D layout (kh,kw,in,out): same names, order and element counts."""
    swap = {"d1_w": (3, 3, gf_dim * 4, gf_dim * 2), "d2_w": (3, 3, gf_dim * 2, gf_dim)}
    return [(n, swap.get(n, s)) for n, s in O.generator_param_shapes(gf_dim, in_c, out_c, n_blocks)]


def generator_resnet_resize(tape, P, x: O.Var, mode, n_blocks=9, eps=1e-3) -> O.Var:
    """O.generator_resnet with the two transposed layers replaced by U -> Conv2D 3x3 stride 1 SAME + bias -> IN -> ReLU."""
    def cin(name, h, stride=1, padding="VALID", reflect=0):
        h = O.conv2d(tape, h, P[name + "_w"], P[name + "_b"], stride, padding, reflect)
        return O.instance_norm(tape, h, P[name + "_g"], P[name + "_beta"], eps)

    h = O.relu(tape, cin("c1", x, reflect=3))
    h = O.relu(tape, cin("c2", h, 2, "SAME"))
    h = O.relu(tape, cin("c3", h, 2, "SAME"))
    for i in range(1, n_blocks + 1):
        y = O.relu(tape, cin(f"r{i}a", h, reflect=1))
        y = cin(f"r{i}b", y, reflect=1)
        h = O.add(tape, y, h)
    for name in ("d1", "d2"):
        h = O.relu(tape, cin(name, upsample2x(tape, h, mode), 1, "SAME"))
    h = O.conv2d(tape, h, P["out_w"], P["out_b"], 1, "VALID", 3)
    return O.tanh(tape, h)


def _grads(tape, loss, inputs, nets, which):
    for v in inputs + [p for n in nets.values() for p in n.values()] + [o for o, _ in tape.ops]:
        v.g = None
    tape.backward([(loss, 1.0)])
    return {n: {k: (np.zeros_like(v.v) if v.g is None else v.g.copy()) for k, v in nets[n].items()} for n in which}


def _adam(params, G, t, lr, beta1):
    return {n: {k: O.adam_tf(P[k], G[n][k], np.zeros_like(P[k]), np.zeros_like(P[k]), t, lr, beta1)[0] for k in P} for n, P in params.items()}


def train_step(generator, PG, PD, real_A, seg_A, mask_A, t=1, lr=1e-3, beta1=0.5, leak=0.3, eps=1e-3, l1_lambda=100.0, signs=None,
               device=None):
    """O.train_step (model.py:169-200) with ``generator(tape, VG, x)`` handed in; first step of fresh Adam slots.  signs, device:
    a SignPolicy and the device's {"fake_A"} for the L1 term's kinks."""
    tape = O.Tape()
    VG, VD = {k: O.Var(v, k) for k, v in PG.items()}, {k: O.Var(v, k) for k, v in PD.items()}
    xA, seg = O.Var(real_A), O.Var(seg_A)
    fake = generator(tape, VG, xA)
    da_real = O.discriminator(tape, VD, seg, mask_A, leak, eps)
    da_fake = O.discriminator(tape, VD, fake, mask_A, leak, eps)
    gen_loss = O.scale_add(tape, O.bce_logits_mean(tape, da_fake, 1.0), l1_mean(tape, np.asarray(seg_A, F64), fake, signs, device and device["fake_A"]), l1_lambda)
    disc_loss = O.scale_add(tape, O.bce_logits_mean(tape, da_real, 1.0), O.bce_logits_mean(tape, da_fake, 0.0), 1.0)
    nets = {"G": VG, "D": VD}
    def regrad():
        G = _grads(tape, gen_loss, [xA, seg], nets, ("G",))
        G.update(_grads(tape, disc_loss, [xA, seg], nets, ("D",)))
        return G

    G = regrad()
    new = _adam({"G": PG, "D": PD}, G, t, lr, beta1)
    return {"fake_A": fake.v, "da_real": da_real.v, "da_fake": da_fake.v, "gen_loss": float(gen_loss.v),
            "disc_loss": float(disc_loss.v), "gG": G["G"], "gD": G["D"], "PG": new["G"], "PD": new["D"], "grads": G, "regrad": regrad}


def cycle_step(generator, PGab, PGba, PDa, PDb, real_A, real_B, seg_A, seg_B, mask_A, mask_B, t=1, lr=2e-4, beta1=0.5,
               L1_lambda=10.0, Lg_lambda=5.0, use_lsgan=True, leak=0.3, eps=1e-3, signs=None, device=None):
    """O.cycle_step with ``generator(tape, V, x)`` handed in; first step of fresh Adam slots.  signs, device: a SignPolicy and the
    device's {"fake_A", "fake_B", "cyc_A", "cyc_B"} for the kinks of the L1 and gradient-sensitive terms."""
    dv = device or {"fake_A": None, "fake_B": None, "cyc_A": None, "cyc_B": None}
    tape = O.Tape()
    V = lambda P: {k: O.Var(v, k) for k, v in P.items()}
    Gab, Gba, Da, Db = V(PGab), V(PGba), V(PDa), V(PDb)
    xA, xB = O.Var(real_A), O.Var(real_B)
    fake_B = generator(tape, Gab, xA)
    cyc_A = generator(tape, Gba, fake_B)
    fake_A = generator(tape, Gba, xB)
    cyc_B = generator(tape, Gab, fake_A)
    DB_fake = O.discriminator(tape, Db, fake_B, mask_A, leak, eps)
    DA_fake = O.discriminator(tape, Da, fake_A, mask_B, leak, eps)
    DA_real = O.discriminator(tape, Da, xA, mask_A, leak, eps)
    DB_real = O.discriminator(tape, Db, xB, mask_B, leak, eps)
    crit = (lambda x, z: O.mse_const_mean(tape, x, z)) if use_lsgan else (lambda x, z: O.bce_logits_mean(tape, x, z))
    wA, wB = O.seg_edge_weight(seg_A), O.seg_edge_weight(seg_B)
    g_loss = O.add_scalars(tape, [
        (1.0, crit(DA_fake, 1.0)), (1.0, crit(DB_fake, 1.0)),
        (L1_lambda, l1_mean(tape, np.asarray(real_A, F64), cyc_A, signs, dv["cyc_A"])),
        (L1_lambda, l1_mean(tape, np.asarray(real_B, F64), cyc_B, signs, dv["cyc_B"])),
        (Lg_lambda, gradloss(tape, fake_A, real_B, wB, signs, dv["fake_A"])), (Lg_lambda, gradloss(tape, fake_B, real_A, wA, signs, dv["fake_B"]))])
    d_loss = O.add_scalars(tape, [(0.5, crit(DA_real, 1.0)), (0.5, crit(DA_fake, 0.0)),
                                  (0.5, crit(DB_real, 1.0)), (0.5, crit(DB_fake, 0.0))])
    nets = {"Gab": Gab, "Gba": Gba, "Da": Da, "Db": Db}
    def regrad():
        G = _grads(tape, g_loss, [xA, xB], nets, ("Gab", "Gba"))
        G.update(_grads(tape, d_loss, [xA, xB], nets, ("Da", "Db")))
        return G

    G = regrad()
    new = _adam({"Gab": PGab, "Gba": PGba, "Da": PDa, "Db": PDb}, G, t, lr, beta1)
    return {"fake_A": fake_A.v, "fake_B": fake_B.v, "cyc_A": cyc_A.v, "cyc_B": cyc_B.v, "g_loss": float(g_loss.v),
            "d_loss": float(d_loss.v), "grads": G, "params": new, "regrad": regrad}
