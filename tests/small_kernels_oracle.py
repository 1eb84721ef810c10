"""NumPy float64 statements of the small kernels of csrc/misc.hip (Adam: csrc/adam.hip), written from include/sggan.h (not from the kernels):
column sum, L1 loss, BCE-with-logits, the LSGAN criterion, the Sobel gradient loss, the segmentation-edge indicator,
channel pad / unpad, the argmax-u8 label rule, the confusion histogram, the activations and Keras-form Adam.

Tensors are pixel-major with the PADDED channel count last, as the C ABI sees them; every function takes the values the
kernel receives (already rounded to the storage type) as float64 and returns float64 (or integers).  Scalars that the ABI
takes as `float` are rounded to float32 first, so that the oracle states the operation on the kernel's actual arguments.

The second half builds the exact-by-construction inputs of tests/test_gpu_small_kernels.py -- values k/8, weights in
{0, 0.5, 1}, power-of-two scalar factors -- and states the premise that makes them exact (`exact_sum_premise`);
tests/test_small_kernels_oracle_cpu.py checks that premise for every case the GPU tests use."""
import numpy as np

F64 = np.float64


def f32(x):
    """The value a C `float` argument holds."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------- the operations
def colsum(dy, C_real):
    """sgg_bias_grad: db[c] = sum_p dy[p][c], c < C_real.  dy (..., C)."""
    dy = np.asarray(dy, F64)
    return dy.reshape(-1, dy.shape[-1]).sum(axis=0)[:C_real]


def l1_sum(a, b, C_real):
    """sum over pixels and real channels of |a - b| (the float64 sum the loss is a multiple of)."""
    d = np.asarray(a, F64)[..., :C_real] - np.asarray(b, F64)[..., :C_real]
    return np.abs(d).sum()


def l1_loss(a, b, C_real, weight=1.0, gscale=1.0):
    """sgg_l1_loss: loss = weight * mean_{p, c < C_real} |a - b|;  db = -weight * gscale * sign(a - b) / (P * C_real),
    0 in padded channels (sign(0) = 0)."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    Cp = a.shape[-1]
    cnt = (a.size // Cp) * C_real
    scale = f32(weight) / cnt
    d = a - b
    db = np.zeros_like(a)
    db[..., :C_real] = -(f32(weight) * f32(gscale) / cnt) * np.sign(d[..., :C_real])
    return l1_sum(a, b, C_real) * scale, db


def sigmoid(x):
    x = np.asarray(x, F64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_logits(x, label, weight=1.0, gscale=1.0):
    """sgg_bce_logits: loss = weight * mean(max(x,0) - x*label + log1p(exp(-|x|)));
    dx = weight * gscale * (sigmoid(x) - label) / n."""
    x = np.asarray(x, F64)
    label, weight, gscale = f32(label), f32(weight), f32(gscale)
    per = np.maximum(x, 0) - x * label + np.log1p(np.exp(-np.abs(x)))
    return weight * per.mean(), weight * gscale * (sigmoid(x) - label) / x.size


def mse_const(x, target, weight=1.0, gscale=1.0):
    """sgg_mse_const: loss = weight * mean((x - t)^2);  dx = weight * gscale * 2 (x - t) / n."""
    x = np.asarray(x, F64)
    target, weight, gscale = f32(target), f32(weight), f32(gscale)
    d = x - target
    return weight * (d * d).mean(), weight * gscale * 2 * d / x.size


SOBEL_X = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], F64)
SOBEL_Y = SOBEL_X.T.copy()


def sobel(x):
    """Depthwise 3x3 correlation with SOBEL_X / SOBEL_Y, SAME zero padding.  x (N,H,W,C) -> (gx, gy)."""
    N, H, W, C = x.shape
    xp = np.zeros((N, H + 2, W + 2, C), F64)
    xp[:, 1:H + 1, 1:W + 1] = x
    gx, gy = np.zeros(x.shape, F64), np.zeros(x.shape, F64)
    for r in range(3):
        for s in range(3):
            win = xp[:, r:r + H, s:s + W]
            gx += SOBEL_X[r, s] * win
            gy += SOBEL_Y[r, s] * win
    return gx, gy


def sobel_transpose(cx, cy):
    """d/dx of sum(cx * gx + cy * gy) for (gx, gy) = sobel(x)."""
    N, H, W, C = cx.shape
    gp = np.zeros((N, H + 2, W + 2, C), F64)
    for r in range(3):
        for s in range(3):
            gp[:, r:r + H, s:s + W] += SOBEL_X[r, s] * cx + SOBEL_Y[r, s] * cy
    return gp[:, 1:H + 1, 1:W + 1]


def gradloss_terms(in_, target, weight, C_real):
    """Per pixel: weight * sum_{c < C_real} ( | |gx(in)| - |gx(target)| | + | |gy(in)| - |gy(target)| | ), (N,H,W)."""
    ax, ay = sobel(np.asarray(in_, F64)[..., :C_real])
    bx, by = sobel(np.asarray(target, F64)[..., :C_real])
    return np.asarray(weight, F64) * (np.abs(np.abs(ax) - np.abs(bx)) + np.abs(np.abs(ay) - np.abs(by))).sum(-1)


def gradloss(in_, target, weight, C_real, lam=1.0, gscale=1.0):
    """sgg_gradloss: loss = lambda * mean_pixels(weight * mean_{2 C_real} | |d(in)| - |d(target)| |);
    din = gscale * d(lambda * loss) / d(in), 0 in padded channels; sign(0) = 0."""
    in_, target, weight = np.asarray(in_, F64), np.asarray(target, F64), np.asarray(weight, F64)
    N, H, W, Cp = in_.shape
    denom = N * H * W * 2.0 * C_real
    lam, gscale = f32(lam), f32(gscale)
    loss = gradloss_terms(in_, target, weight, C_real).sum() * (lam / denom)
    ax, ay = sobel(in_[..., :C_real])
    bx, by = sobel(target[..., :C_real])
    k = (lam * gscale / denom) * weight[..., None]
    cx = k * np.sign(np.abs(ax) - np.abs(bx)) * np.sign(ax)
    cy = k * np.sign(np.abs(ay) - np.abs(by)) * np.sign(ay)
    din = np.zeros_like(in_)
    din[..., :C_real] = sobel_transpose(cx, cy)
    return loss, din


def seg_edge(seg, C_real):
    """sgg_seg_edge_weight: 1 where the REFLECT-padded map has a non-zero central difference in x or y on a real channel."""
    s = np.asarray(seg, F64)[..., :C_real]
    sp = np.pad(s, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="reflect")
    dx = sp[:, 1:-1, 2:] - sp[:, 1:-1, :-2]
    dy = sp[:, 2:, 1:-1] - sp[:, :-2, 1:-1]
    return ((np.abs(dx) + np.abs(dy)).sum(-1) > 0).astype(F64)


def pad_channels(x, Cd):
    """[P][Cs] -> [P][Cd], zero fill."""
    x = np.asarray(x, F64)
    out = np.zeros(x.shape[:-1] + (Cd,), F64)
    out[..., :x.shape[-1]] = x
    return out


def unpad_channels(x, Cd):
    return np.asarray(x, F64)[..., :Cd].copy()


def argmax_u8(x, C_real):
    """labels = argmax_{c < C_real} ( int32(f32(255) * f32(x)) & 0xff ), first maximum wins.  x (P, Cpad) holds values that are
    exact in float32; |255 x| < 2^31."""
    p = np.float32(255) * np.asarray(x)[..., :C_real].astype(np.float32)        # one float32 product
    v = p.astype(np.float64).astype(np.int64).astype(np.int32) & 0xff           # truncate toward zero, low 8 bits
    return np.argmax(v, axis=-1).astype(np.int32)


def confusion_hist(label_true, label_pred, n_class):
    """hist[n_class * t + p] += 1 for pixels with 0 <= t, p < n_class."""
    t, p = np.asarray(label_true, np.int64).ravel(), np.asarray(label_pred, np.int64).ravel()
    ok = (t >= 0) & (t < n_class) & (p >= 0) & (p < n_class)
    return np.bincount(n_class * t[ok] + p[ok], minlength=n_class * n_class).astype(np.int64)


def act_fwd(x, act, leak=0.0):
    x = np.asarray(x, F64)
    if act == "relu":
        return np.where(x > 0, x, 0.0)
    if act == "lrelu":
        return np.where(x > 0, x, f32(leak) * x)
    if act == "tanh":
        return np.tanh(x)
    return x.copy()


def act_bwd(dy, y, act, leak=0.0):
    """dx = dy * act'(.) evaluated from the OUTPUT y (relu / lrelu: sign of y; tanh: 1 - y^2)."""
    dy, y = np.asarray(dy, F64), np.asarray(y, F64)
    if act == "relu":
        return dy * (y > 0)
    if act == "lrelu":
        return dy * np.where(y > 0, 1.0, f32(leak))
    if act == "tanh":
        return dy * (1.0 - y * y)
    return dy.copy()


def adam(theta, g, m, v, t, lr=1e-3, beta1=0.5, beta2=0.999, eps=1e-7, grad_scale=1.0):
    """Keras form: g *= grad_scale; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
    theta -= lr sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)."""
    lr, beta1, beta2, eps, grad_scale = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(grad_scale)
    g = np.asarray(g, F64) * grad_scale
    m = beta1 * np.asarray(m, F64) + (1 - beta1) * g
    v = beta2 * np.asarray(v, F64) + (1 - beta2) * g * g
    lr_t = lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    return np.asarray(theta, F64) - lr_t * m / (np.sqrt(v) + eps), m, v


# ---------------------------------------------------------------------------- exact-by-construction inputs
# Values k/8 with |k| <= 8 and weights in {0, 0.5, 1} are exact in bfloat16 and float32, and so is every difference, Sobel
# derivative and product the kernels form from them.  A float32 sum of such terms is exact in ANY order as long as the sum of
# their magnitudes stays below 2^24 units of their common granule; the kernels add float32 only within one chunk / one
# block and combine the chunks in double, so the premise is checked per chunk (exact_sum_premise).

def eighths(rng, shape):
    """Random values k/8, |k| <= 8."""
    return rng.integers(-8, 9, shape).astype(F64) / 8.0


def half_weights(rng, shape):
    return rng.integers(0, 3, shape).astype(F64) / 2.0


def pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


def pow2_factor(count):
    """(scalar, factor): the float32 scalar argument (L1 weight, grad-loss lambda) for which scalar / count is the power of
    two `factor` = 1 / pow2_at_least(count) exactly.  count < 2^24, so scalar = count * factor is exact in float32."""
    assert 0 < count < 2 ** 24
    factor = 1.0 / pow2_at_least(count)
    scalar = count * factor
    assert float(np.float32(scalar)) == scalar and scalar / count == factor
    return scalar, factor


def exact_sum_premise(terms, groups, granule):
    """terms: float64 (n,) or (n, k) -- the addends in the order the kernel meets them (k independent columns); groups: list of
    index arrays into axis 0, one per float32 accumulator chain (a chunk / a block), the rest of the reduction being double.
    Checks that (1) every term is an integer multiple of `granule`, (2) within each group the magnitudes add up to less than
    2^24 granules, so that every float32 partial sum in any order is exact, (3) the float32 running sum of each group, term
    by term, equals the float64 one bit for bit, and (4) the double combination of the groups equals the float64 sum of all
    terms.  Returns that sum (per column)."""
    terms = np.asarray(terms, F64)
    terms = terms.reshape(terms.shape[0], -1)
    q = terms / granule
    assert np.array_equal(q, np.round(q)), "terms are not multiples of the granule"
    total = np.zeros(terms.shape[1], F64)
    seen = 0
    for idx in groups:
        t = terms[idx]
        if not len(t):
            continue
        assert (np.abs(t).sum(axis=0) / granule).max() < 2 ** 24, "a float32 partial sum may need more than 24 bits"
        run32 = np.cumsum(t.astype(np.float32), axis=0, dtype=np.float32)
        assert np.array_equal(run32.astype(F64), np.cumsum(t, axis=0)), "float32 running sum differs from float64"
        total += run32[-1].astype(F64)
        seen += len(t)
    assert seen == terms.shape[0], "groups do not cover the terms"
    assert np.array_equal(total, terms.sum(axis=0)) and (np.abs(total) / granule).max() < 2 ** 53
    return total if total.size > 1 else float(total[0])


def chunk_groups(n, rows):
    """Index groups of a reduction that walks n items in consecutive chunks of `rows` (one float32 partial per chunk)."""
    return [np.arange(i, min(i + rows, n)) for i in range(0, n, rows)]


def grid_stride_groups(n, block, max_blocks):
    """Index groups of a grid-stride reduction: thread (b, t) of min(ceil(n / block), max_blocks) blocks takes items
    b * block + t + k * blocks * block; one float32 partial per block."""
    blocks = min((n + block - 1) // block, max_blocks)
    idx = np.arange(n)
    owner = (idx % (blocks * block)) // block
    order = np.argsort(owner, kind="stable")
    return np.split(order, np.searchsorted(owner[order], np.arange(1, blocks)))


# ---------------------------------------------------------------------------- the cases both test files use
# Chunk sizes as the workspace functions of include/sggan.h imply them: sgg_bias_grad_workspace = ceil(P / 1024) rows of C floats,
# sgg_l1_loss_workspace = ceil(P * Cpad / 4 / 2048) floats, sgg_gradloss_workspace = the coefficients + 1024 block partials.
BG_ROWS, L1_ROWS, GL_BLOCKS, BLOCK = 1024, 2048, 1024, 256
VEC = {"f32": 4, "bf16": 8}                    # elements per 16-byte vector

BIAS_C = {"f32": (8, 40, 24, 520, 1032), "bf16": (8, 40, 520, 2056)}
BIAS_P = (1, 1023, 1024, 1025, 3000)
BIAS_P_BIG = 262144 + 1024 + 5                 # more than 256 chunks, ragged; C = 8


def bias_case(C, P, seed=0):
    return eighths(np.random.default_rng([11, C, P, seed]), (P, C))


L1_SHAPES = ((3, 8), (10, 16), (8, 8))         # (C_real, Cpad)
L1_NVEC = (1, 2047, 2048, 2049, 5000)
L1_P_BIG = 262147                              # Cpad 8, f32: 524294 vectors = more than 256 chunks


def l1_pixels(nvec, Cp, dtype):
    """The smallest pixel count whose tensor has at least `nvec` 16-byte vectors."""
    return max(1, -(-nvec * VEC[dtype] // Cp))


def l1_case(P, Cr, Cp, seed=0):
    """a, b (P, Cp) in eighths, about a quarter of the entries tied; the padded channels differ too (the kernel must not count
    them).  weight is chosen so that weight / (P * Cr) is a power of two."""
    rng = np.random.default_rng([12, P, Cr, Cp, seed])
    a, b = eighths(rng, (P, Cp)), eighths(rng, (P, Cp))
    tie = rng.integers(0, 4, (P, Cp)) == 0
    tie[0, 0] = True                              # at least one tie in a real channel, also at P = 1
    b[tie] = a[tie]
    weight, factor = pow2_factor(P * Cr)
    return a, b, weight, factor


def l1_terms(a, b, Cr):
    """The addends in memory order: |a - b| in real channels, 0 in padded ones."""
    d = np.abs(a - b)
    d[..., Cr:] = 0.0
    return d.ravel()


GL_VEC_SHAPES = ((3, 8), (4, 8), (1, 8), (3, 16))      # C_real <= 4 and 8 | Cpad: one thread per pixel, 16-byte loads
GL_SCALAR_SHAPES = ((3, 4), (5, 8))                    # (3, 4): float32 only (Cpad is no multiple of 8)
GL_DIMS = ((1, 1, 1), (1, 1, 7), (1, 7, 1), (3, 2, 5), (2, 16, 24))
GL_DIMS_BIG = (1, 513, 512)                            # more pixels than 1024 blocks x 256 threads


def gradloss_case(N, H, W, Cr, Cp, seed=0):
    """in, target (N,H,W,Cp) in eighths (every image different, padded channels non-zero), weight (N,H,W) in {0, 0.5, 1},
    lambda such that lambda / (N*H*W*2*Cr) is a power of two."""
    rng = np.random.default_rng([13, N, H, W, Cr, Cp, seed])
    a, b = eighths(rng, (N, H, W, Cp)), eighths(rng, (N, H, W, Cp))
    w = half_weights(rng, (N, H, W))
    lam, factor = pow2_factor(N * H * W * 2 * Cr)
    return a, b, w, lam, factor
