"""NumPy float64 statement of instance normalisation as include/sggan.h declares it (sgg_instnorm_*), written from the header
and the formula of oracle/sggan_oracle.py::instance_norm -- not from csrc/norm.hip -- plus the ERROR BOUNDS that the arithmetic
promised by the header and norm.hip's opening comment implies, and the inputs of tests/test_gpu_instnorm.py.

Tensors are (N, H, W, C) with the padded channel count last; every array holds the values the kernel receives (already rounded
to the storage type) as float64.  `eps` and `leak` are rounded to float32 first, as the ABI takes them.

The operation (per image n and channel c, over the HW pixels; biased variance):
    mean = E[x]   var = E[(x - mean)^2]   rstd = 1 / sqrt(var + eps)   xhat = (x - mean) * rstd
    plain form:  y = act(gamma * xhat + beta) (+ residual, after the activation)
    skip form :  y = act(gamma * xhat + beta + skip)
    act: NONE, RELU, LRELU(leak); the slope at a pre-activation of exactly 0 is 0 (RELU) / leak (LRELU): the kernels test `> 0`
    backward  :  g = dy * act'(pre);  dskip = g;  dbeta = sum g;  dgamma = sum g * xhat  (over n and the pixels)
                 dx = gamma * rstd * (g - E[g] - xhat * E[g * xhat])
    two networks in lockstep ("pair"): images n < nsplit use (gamma, beta), the rest (gamma2, beta2); the parameter gradients
    are summed per set.

The arithmetic the bounds are derived from (u = 2^-24, the float32 unit roundoff; -ffp-contract=off, so no fused operations):
    * elementwise operations are float32, each with relative error <= u;
    * the statistics sums (sum x, sum x^2; backward: sum g, sum g*xhat) are float64 on the f32 path and rounded to float32 ONCE
      per pixel chunk (relative error u of that chunk's sum of magnitudes; the float64 accumulation adds n * 2^-53, also
      counted); the chunks are combined in float64.  On the bf16 path the sums within a chunk are float32 in an order the
      header does not fix: any order of n float32 additions (and one product rounding) is within n * u of the sum of
      magnitudes.  `sum_rel(name, n)` is that relative error.  Maps of at most FUSED_MAXHW pixels are done in one launch, the
      whole image being one chunk; larger ones in chunks of rows_per_chunk(HW) pixels (sgg_instnorm_workspace counts them);
    * mean and rstd are formed in float64 from the combined sums and stored as float32 (one rounding, u);
    * the result is rounded to the storage type once: 2^-8 relative for bfloat16 (8 significant bits, round to nearest even), nothing more for f32.
Every bound below is the first-order propagation of these elementary errors (rstd: the exact interval), times ONE safety
factor SAFETY shared by all outputs and cases (it covers the second-order terms).  The tests assert err <= bound per element
(stats: per (n, c)); nothing is judged by a maximum over the tensor's scale."""
import functools
import itertools

import numpy as np

F64 = np.float64
U32 = 2.0 ** -24
USTORE = {"f32": 0.0, "bf16": 2.0 ** -8}        # bfloat16 keeps 8 significant bits: half an ulp is 2^-8 relative
SAFETY = 4.0                                   # the one constant (the issue allows at most 8)
FUSED_MAXHW = 512                              # one-launch path up to here (plain forward / backward and their pair forms)
NONE, RELU, LRELU, TANH = 0, 1, 2, 3


def f32(v):
    """The value a C `float` argument holds."""
    return float(np.float32(v))


def rows_per_chunk(HW):
    """Pixels per statistics chunk: at least 64, a multiple of 64, at most ~128 chunks per image, at most 4096."""
    r = (HW + 127) // 128
    r = (r + 63) // 64 * 64
    return int(min(max(r, 64), 4096))


def chunks(HW):
    return -(-HW // rows_per_chunk(HW))


def rows_per_block(N, HW):
    """Pixels per block of the apply passes (>= 2048 blocks of >= 64 pixels); only the shape table's reasons quote it."""
    return int(min(max(HW * N // 2048, 64), 4096))


def chain_pixels(HW, one_launch):
    """Pixels that one chunk's sums cover: the whole image on the one-launch path, rows_per_chunk(HW) otherwise."""
    return HW if (one_launch and HW <= FUSED_MAXHW) else min(HW, rows_per_chunk(HW))


def sum_rel(name, npix):
    """Relative error (of the sum of magnitudes) of one chunk's sum as handed to the float64 combination."""
    return U32 + npix * 2.0 ** -53 if name == "f32" else npix * U32


def slope(pre, act, leak):
    pre = np.asarray(pre, F64)
    if act == RELU:
        return (pre > 0).astype(F64)
    if act == LRELU:
        return np.where(pre > 0, 1.0, f32(leak))
    return np.ones_like(pre)


def act_fwd(pre, act, leak):
    return np.asarray(pre, F64) * slope(pre, act, leak)


def per_image(p, N, pair=None, second=None):
    """(N, 1, 1, C) parameter array: p for every image, or p / second picked by image index (pair = nsplit)."""
    p = np.asarray(p, F64)
    out = np.repeat(p[None], N, axis=0)
    if pair is not None:
        out[pair:] = np.asarray(second, F64)
    return out[:, None, None, :]


# ---------------------------------------------------------------------------- the operation
def stats(x, eps):
    """(mean, rstd), each (N, C), float64."""
    x = np.asarray(x, F64)
    mean = x.mean((1, 2))
    var = ((x - mean[:, None, None, :]) ** 2).mean((1, 2))
    return mean, 1.0 / np.sqrt(var + f32(eps))


def forward(x, gamma, beta, eps=1e-3, act=NONE, leak=0.0, residual=None, skip=None, pair=None):
    """-> (y, mean, rstd, pre).  gamma / beta: (C,), or pair = (gamma2, beta2, nsplit).  pre is the activation's argument."""
    x = np.asarray(x, F64)
    N = x.shape[0]
    g = per_image(gamma, N, *(pair[2], pair[0]) if pair else ())
    b = per_image(beta, N, *(pair[2], pair[1]) if pair else ())
    mean, rstd = stats(x, eps)
    pre = g * (x - mean[:, None, None, :]) * rstd[:, None, None, :] + b
    if skip is not None:
        pre = pre + np.asarray(skip, F64)
    y = act_fwd(pre, act, leak)
    if residual is not None:
        y = y + np.asarray(residual, F64)
    return y, mean, rstd, pre


def backward(dy, x, gamma, beta, mean, rstd, act=NONE, leak=0.0, skip=None, pair=None):
    """Given (mean, rstd) as the forward wrote them -> dict(dx, dskip, dgamma, dbeta[, dgamma2, dbeta2]).  dskip = g is the skip
    path's gradient (meaningful for the skip form)."""
    dy, x = np.asarray(dy, F64), np.asarray(x, F64)
    N, H, W, C = x.shape
    gm = per_image(gamma, N, *(pair[2], pair[0]) if pair else ())
    bt = per_image(beta, N, *(pair[2], pair[1]) if pair else ())
    mu, rs = np.asarray(mean, F64)[:, None, None, :], np.asarray(rstd, F64)[:, None, None, :]
    xh = (x - mu) * rs
    pre = gm * xh + bt + (0.0 if skip is None else np.asarray(skip, F64))
    g = dy * slope(pre, act, leak)
    m1, m2 = g.mean((1, 2), keepdims=True), (g * xh).mean((1, 2), keepdims=True)
    out = {"dx": gm * rs * (g - m1 - xh * m2), "dskip": g, "g": g, "xhat": xh, "pre": pre}
    sg, sgx = g.sum((1, 2)), (g * xh).sum((1, 2))             # (N, C)
    n1 = pair[2] if pair else N
    out["dbeta"], out["dgamma"] = sg[:n1].sum(0), sgx[:n1].sum(0)
    if pair:
        out["dbeta2"], out["dgamma2"] = sg[n1:].sum(0), sgx[n1:].sum(0)
    return out


def _rows(a, b, nchunks):
    N, H, W, C = a.shape
    a, b = a.reshape(N, H * W, C), b.reshape(N, H * W, C)
    out = np.zeros((N, nchunks, C, 2), F64)
    for k, idx in enumerate(np.array_split(np.arange(H * W), nchunks)):
        out[:, k, :, 0], out[:, k, :, 1] = a[:, idx].sum(1), b[:, idx].sum(1)
    return out.astype(np.float32)


def partial_rows(x, nchunks):
    """partial[N][nchunks][C][2] = per-chunk (sum x, sum x^2), float64 sums cast to float32, for ANY chunk count (consecutive
    pixel ranges as even as possible; more chunks than pixels leaves empty chunks, which are 0)."""
    x = np.asarray(x, F64)
    return _rows(x, x * x, nchunks)


def bwd_partial_rows(dy, x, gamma, beta, mean, rstd, act, leak, nchunks, pair=None):
    """The backward analogue: per-chunk (sum g, sum g * xhat) for sgg_instnorm_bwd_partial."""
    b = backward(dy, x, gamma, beta, mean, rstd, act, leak, pair=pair)
    return _rows(b["g"], b["g"] * b["xhat"], nchunks)


def finalize(partial, HW, eps):
    """(mean, rstd) from statistics rows, in float64 (var clamped at 0)."""
    s = np.asarray(partial, F64).sum(1)
    mean = s[..., 0] / HW
    var = np.maximum(s[..., 1] / HW - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + f32(eps))


# ---------------------------------------------------------------------------- the bounds
def stats_bounds(x, eps, rel, k=SAFETY):
    """(bound on mean, bound on rstd), (N, C).  With S1, S2 the combined sums, each chunk's contribution off by rel * (its sum of
    magnitudes):  |d mean'| <= rel * E|x| for the float64 mean', and the stored mean adds u * |mean|;
    var' = S2/HW - mean'^2, so |d var| <= rel * E[x^2] + 2 |mean| rel E|x|  (<= rel * (2 E[x^2] + mean^2): the E[x^2] - mean^2 form
    pays for a large mean in absolute terms).  rstd = (var + eps)^-1/2 is monotone and the clamp var' >= 0 only moves var'
    towards the true var >= 0, so rstd' lies in [(var + d + eps)^-1/2, (max(var - d, 0) + eps)^-1/2]; the bound is the larger
    distance to an end of that interval (no linearisation: d may exceed var + eps) plus u * rstd for the float32 store."""
    x = np.asarray(x, F64)
    eps, u, r = f32(eps), k * U32, k * rel
    mean = x.mean((1, 2))
    var = ((x - mean[:, None, None, :]) ** 2).mean((1, 2))
    e1, e2 = np.abs(x).mean((1, 2)), (x * x).mean((1, 2))
    dmean = r * e1 + u * np.abs(mean)
    dvar = r * e2 + 2 * np.abs(mean) * r * e1
    rstd = 1 / np.sqrt(var + eps)
    hi, lo = 1 / np.sqrt(np.maximum(var - dvar, 0.0) + eps), 1 / np.sqrt(var + dvar + eps)
    return dmean, np.maximum(hi - rstd, rstd - lo) * (1 + u) + u * rstd


def forward_bounds(x, gamma, beta, eps, act, leak, name, rel, residual=None, skip=None, pair=None, k=SAFETY):
    """Elementwise bound on y (and on the pre-activation, for the kink margin) -> (by, bpre).
    The kernel forms A = gamma * rstd', B = beta - mean' * A, pre = x * A + B -- in exact arithmetic A' (x - mean') + beta -- so
        |d pre| <= dA |x - mean| + |A| dmean                       (the statistics' errors; dA = |gamma| drstd + u |A|)
                 + u (|mean A| + |B| + |x A| + |pre|)               (the four float32 roundings; the |x A| term is what a
                                                                     large mean costs although the result is small)
                 + u |pre + skip|                                   (skip form: one more addition)
    RELU and LRELU are 1-Lipschitz whichever side of the kink either value is on; LRELU's product adds u |y|, the residual
    addition u |y|, the store to the tensor's type ustore * |y|."""
    x = np.asarray(x, F64)
    N = x.shape[0]
    u, s = k * U32, k * USTORE[name]
    y, mean, rstd, pre = forward(x, gamma, beta, eps, act, leak, residual, skip, pair)
    dmean, drstd = stats_bounds(x, eps, rel, k)
    g = per_image(gamma, N, *(pair[2], pair[0]) if pair else ())
    b = per_image(beta, N, *(pair[2], pair[1]) if pair else ())
    mu, rs, dmu, drs = (a[:, None, None, :] for a in (mean, rstd, dmean, drstd))
    A = g * rs
    B = b - mu * A
    dA = np.abs(g) * drs + u * np.abs(A)
    z = x * A + B
    bpre = dA * np.abs(x - mu) + np.abs(A) * dmu + u * (np.abs(mu * A) + np.abs(B) + np.abs(x * A) + np.abs(z))
    if skip is not None:
        bpre = bpre + u * np.abs(pre)
    by = bpre.copy()
    y0 = act_fwd(pre, act, leak)
    if act == LRELU:
        by += u * np.abs(y0)
    if residual is not None:
        by += u * np.abs(y)
    by += s * (np.abs(y) + by)
    return by, bpre


def backward_bounds(dy, x, gamma, beta, mean, rstd, act, leak, name, rel, dmean_in=None, drstd_in=None, skip=None, pair=None,
                    store_g=False, accumulate_onto=None, k=SAFETY):
    """Elementwise bounds on dx / dskip and per-channel bounds on the parameter gradients, for a backward that is handed
    (mean, rstd) off by at most (dmean_in, drstd_in) -- default: the oracle's values rounded to float32.
        xhat' = ((x - mean') rstd'):   dxh = rstd (dmean + u |x - mean|) + |x - mean| drstd + u |xhat|
        g' = dy * slope:               dg = u |g|  (+ ustore |g| where the skip form stores dskip and sums the stored values);
                                       the slope itself is the oracle's: the builders keep every pre-activation 64 forward
                                       bounds away from 0 (returned as `bpre`: the bound on the backward's own pre-activation)
        m1 = E[g], m2 = E[g xhat]:     dm1 = rel E|g| + E[dg] + u |m1|
                                       dm2 = (rel + u) E|g xhat| + E[|g| dxh + dg |xhat|] + u |m2|
        t = (g - m1) - xhat m2:        dt = dg + dm1 + u |g - m1| + |m2| dxh + |xhat| dm2 + u |xhat m2| + u |t|
        dx = A t, A = gamma rstd':     ddx = dA |t| + |A| dt + (u + ustore) |dx|,   dA = |gamma| drstd + u |A|
        dbeta = sum_n f32(S_g(n)), dgamma = sum_n f32(S_gx(n)):  HW times the sums' parts of dm1 / dm2, u |S| for each image's
                                       float32 total, u |result| for the final cast (and for the addition when accumulating)."""
    dy, x = np.asarray(dy, F64), np.asarray(x, F64)
    N, H, W, C = x.shape
    HW = H * W
    u, s, r = k * U32, k * USTORE[name], k * rel
    o = backward(dy, x, gamma, beta, mean, rstd, act, leak, skip, pair)
    gm = per_image(gamma, N, *(pair[2], pair[0]) if pair else ())
    mean, rstd = np.asarray(mean, F64), np.asarray(rstd, F64)
    dmean = u * np.abs(mean) if dmean_in is None else np.asarray(dmean_in, F64)
    drstd = u * np.abs(rstd) if drstd_in is None else np.asarray(drstd_in, F64)
    mu, rs, dmu, drs = (a[:, None, None, :] for a in (mean, rstd, dmean, drstd))
    g, xh = o["g"], o["xhat"]
    xc = np.abs(x - mu)
    dxh = rs * (dmu + u * xc) + xc * drs + u * np.abs(xh)
    bpre = np.abs(gm) * dxh + u * np.abs(gm * xh) + u * np.abs(o["pre"])
    dg = (u + (s if store_g else 0.0)) * np.abs(g)
    mean_ = lambda a: a.mean((1, 2), keepdims=True)
    m1, m2 = mean_(g), mean_(g * xh)
    e1, e2 = mean_(np.abs(g)), mean_(np.abs(g * xh))
    sum1 = r * e1 + mean_(dg)
    sum2 = (r + u) * e2 + mean_(np.abs(g) * dxh + dg * np.abs(xh))
    dm1, dm2 = sum1 + u * np.abs(m1), sum2 + u * np.abs(m2)
    t = g - m1 - xh * m2
    dt = dg + dm1 + u * np.abs(g - m1) + np.abs(m2) * dxh + np.abs(xh) * dm2 + u * np.abs(xh * m2) + u * np.abs(t)
    A = gm * rs
    dA = np.abs(gm) * drs + u * np.abs(A)
    bdx = dA * np.abs(t) + np.abs(A) * dt + u * np.abs(o["dx"])
    bdx += s * (np.abs(o["dx"]) + bdx)
    bdskip = dg + s * np.abs(g)
    tb = (HW * sum1 + u * np.abs(HW * m1))[:, 0, 0, :]         # per image (N, C)
    tg = (HW * sum2 + u * np.abs(HW * m2))[:, 0, 0, :]
    n1 = pair[2] if pair else N
    out = {"dx": bdx, "dskip": bdskip, "bpre": bpre}
    for key, tot, sl in (("dbeta", tb, slice(0, n1)), ("dgamma", tg, slice(0, n1)), ("dbeta2", tb, slice(n1, N)), ("dgamma2", tg, slice(n1, N))):
        if key in o:
            base = 0.0 if accumulate_onto is None else np.abs(np.asarray(accumulate_onto[key], F64))
            out[key] = tot[sl].sum(0) + u * np.abs(o[key]) + (0.0 if accumulate_onto is None else u * (base + np.abs(o[key])))
    return out


# ---------------------------------------------------------------------------- storage rounding on the host
def to_storage(a, name):
    """float64 values of `a` after rounding to float32 and then (bf16) to bfloat16, round to nearest even."""
    a32 = np.asarray(a, F64).astype(np.float32)
    if name == "f32":
        return a32.astype(F64)
    b = a32.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(F64).reshape(a32.shape)


def ulp(a, name):
    """Spacing of the storage type at |a| (float32: np.spacing; bfloat16: 2^16 float32 spacings)."""
    sp = np.spacing(np.abs(np.asarray(a, F64)).astype(np.float32)).astype(F64)
    return sp if name == "f32" else sp * 65536.0


# ---------------------------------------------------------------------------- the exact family
# Per (n, c) the pixels hold a short integer pattern, repeated and shuffled: zero mean, integer variance v, and eps = 4^j - v,
# so mean = 0, rstd = 2^-j and xhat = x * 2^-j are exact.  gamma is a signed power of two, beta / residual / skip / dy are
# eighths, LRELU's leak is 1/4: every product is exact, every per-chunk sum of x, x^2 (integers <= 16), g (multiples of 1/32,
# |g| <= 2) and g * xhat (multiples of 1/128) is an exact float32 in any order (4096 * 4 * 128 = 2^21 granules), and the
# per-(n, c) constants of dy are searched so that E[g] and E[g xhat] are short dyadic numbers: dx is then exact too.
PATTERNS = {                                  # name: (pattern, eps); var + eps is a power of four
    "zero": ((0,), 4.0), "pm1": ((1, -1), 3.0), "triple": ((-1, -1, 2), 2.0), "five": ((-1, -1, -1, -1, 4), 12.0),
    "zeros": ((2, -2, 0, 0), 2.0),
}
EXACT_LEAK = 0.25


def exact_pattern(HW, want_zeros=False):
    if HW == 1:
        return "zero"
    if want_zeros and HW % 4 == 0:
        return "zeros"
    for nm in ("pm1", "triple", "five"):
        if HW % len(PATTERNS[nm][0]) == 0:
            return nm
    raise ValueError(f"no exact pattern for HW = {HW}")


@functools.lru_cache(maxsize=None)
def _dy_constants(counts, slopes, xhs, HW):
    """All (k_i) in eighths, one per value group, for which M1 = sum n_i s_i k_i / 8L and M2 = sum n_i s_i k_i xh_i / 8L are
    multiples of 2^-10 whose totals HW * M are exact float32 with at most 17 integer bits; both non-zero where that is possible."""
    L = sum(counts)
    good, fallback = [], []
    for ks in itertools.product(range(-8, 9), repeat=len(counts)):
        m1 = sum(n * s * kk for n, s, kk in zip(counts, slopes, ks)) / (8.0 * L)
        m2 = sum(n * s * kk * xh for n, s, kk, xh in zip(counts, slopes, ks, xhs)) / (8.0 * L)
        if (m1 * 1024) % 1 or (m2 * 1024) % 1 or max(abs(m1), abs(m2)) * HW >= 2 ** 17 or f32(m1 * HW) != m1 * HW or f32(m2 * HW) != m2 * HW:
            continue
        (good if m1 != 0 and m2 != 0 else fallback).append(ks)
    return good or fallback


def exact_case(name, N, H, W, C, act, seed=0, want_zeros=False, pair=None):
    """dict of inputs (float64 arrays of storage-exact values): x, gamma, beta, [gamma2, beta2,] residual, skip, dy (for the
    plain backward), dy_skip (for the skip backward), eps, leak, pattern.  In every even channel beta puts one value group of
    the plain form EXACTLY at pre-activation 0, and skip does the same for another group of the skip form."""
    HW = H * W
    pat = exact_pattern(HW, want_zeros)
    vals, eps = PATTERNS[pat]
    rstd = 1.0 / np.sqrt(np.var(vals) + eps)
    rng = np.random.default_rng([21, N, H, W, C, act, seed, int(want_zeros)])
    uniq = sorted(set(vals))
    sign = np.where((np.arange(C) % 3 == 2) & (pat != "zeros"), -1.0, 1.0)      # every third channel holds the mirrored pattern
    x = np.zeros((N, HW, C), F64)
    base = np.tile(np.asarray(vals, F64), HW // len(vals))
    for n in range(N):
        for c in range(C):
            x[n, :, c] = rng.permutation(base) * sign[c]
    pow2 = np.array([1.0, 2.0, 0.5, -1.0, 4.0, -2.0])

    def params(shift):
        gamma = pow2[(np.arange(C) + shift) % len(pow2)]
        beta = np.zeros(C, F64)
        for c in range(C):
            v0 = sign[c] * uniq[(c // 2 + shift) % len(uniq)]
            beta[c] = -gamma[c] * rstd * v0 + (0.0 if c % 2 == 0 else (2 * rng.integers(0, 2) - 1) * 0.125 * (1 + 2 * rng.integers(0, 2)))
        return gamma, beta

    gamma, beta = params(0)
    out = {"name": name, "eps": eps, "leak": EXACT_LEAK, "act": act, "pattern": pat, "gamma": gamma, "beta": beta, "pair": None}
    if pair is not None:
        g2, b2 = params(3)
        out.update(gamma2=g2, beta2=b2, pair=(g2, b2, pair))
    gi = per_image(gamma, N, *(pair, out["gamma2"]) if pair is not None else ())[:, 0]        # (N, 1, C)
    bi = per_image(beta, N, *(pair, out["beta2"]) if pair is not None else ())[:, 0]
    pre = gi * rstd * x + bi
    # skip: a function of the pixel's x value; in even channels it cancels the pre-activation of one group exactly
    skip = np.zeros_like(x)
    for n in range(N):
        for c in range(C):
            for j, v in enumerate(sorted(set(x[n, :, c]))):
                sel = x[n, :, c] == v
                kk = rng.integers(-8, 9) / 8.0
                skip[n, sel, c] = -pre[n, sel, c] if (c % 2 == 0 and j == (c // 2 + 1) % len(uniq)) else kk
    out["residual"] = rng.integers(-8, 9, x.shape) / 8.0

    def make_dy(pre_):
        dy = np.zeros_like(x)
        for n in range(N):
            for c in range(C):
                groups = sorted(set(x[n, :, c]))
                idx = [np.flatnonzero(x[n, :, c] == v) for v in groups]
                sl = tuple(float(slope(pre_[n, i[0], c], act, EXACT_LEAK)) for i in idx)
                cand = _dy_constants(tuple(len(i) * len(vals) // HW for i in idx), sl, tuple(v * rstd for v in groups), HW)
                ks = cand[rng.integers(0, len(cand))]
                for i, kk in zip(idx, ks):
                    a = kk / 8.0
                    d = rng.integers(0, 9, len(i) // 2) / 8.0                 # +d / -d on pairs of pixels with the same x
                    dy[n, i[0:2 * len(d):2], c] = a + d
                    dy[n, i[1:2 * len(d):2], c] = a - d
                    dy[n, i[2 * len(d):], c] = a
        return dy

    out["dy"], out["dy_skip"] = make_dy(pre), make_dy(pre + skip)
    for key in ("residual", "skip", "dy", "dy_skip"):
        out[key] = (skip if key == "skip" else out[key]).reshape(N, H, W, C)
    out["x"] = x.reshape(N, H, W, C)
    return out


def exact_premise(case, kind="x"):
    """The premise of the exact family, asserted: every input is exact in the storage type; per (n, c) the mean is 0 and
    var + eps a power of four; every chunk's sums (for ANY chunking: bounded through the whole image's sum of magnitudes where
    that is below 2^24 granules, else through 4096-pixel chunks) are exact float32; E[g], E[g xhat], each image's totals, the
    parameter gradients and dx are exact float32 numbers.  Returns the oracle's backward dicts (plain, skip)."""
    name, x, eps = case["name"], case["x"], case["eps"]
    N, H, W, C = x.shape
    HW = H * W
    for key in ("x", "residual", "skip", "dy", "dy_skip"):
        assert np.array_equal(to_storage(case[key], "bf16"), case[key]), f"{key} is not exact in bfloat16"
    for key in ("gamma", "beta", "gamma2", "beta2"):
        if key in case:
            assert np.array_equal(case[key].astype(np.float32).astype(F64), case[key])
    assert f32(eps) == eps and f32(case["leak"]) == case["leak"]
    mean, rstd = stats(x, eps)
    assert not mean.any(), "mean is not exactly 0"
    e = np.log2(rstd)
    assert np.array_equal(e, np.round(e)), "rstd is not a power of two"
    assert np.abs(x).max() <= 4 and np.array_equal(x, np.round(x))
    worst = min(HW, 4096)
    assert worst * 16 < 2 ** 24                                   # sum x^2 per chunk, granule 1
    outs = []
    for dyk, skip in (("dy", None), ("dy_skip", case["skip"])):
        o = backward(case[dyk], x, case["gamma"], case["beta"], mean, rstd, case["act"], case["leak"], skip, case["pair"])
        g, xh = o["g"], o["xhat"]
        assert np.array_equal(g * 32, np.round(g * 32)) and np.abs(g).max() <= 2
        assert np.array_equal(xh * 4, np.round(xh * 4)) and np.abs(xh).max() <= 2
        assert worst * 4 * 128 < 2 ** 24                          # sum |g xhat| per chunk in granules of 1/128
        m1, m2 = g.mean((1, 2)), (g * xh).mean((1, 2))
        for m in (m1, m2):
            assert np.array_equal(m * 1024, np.round(m * 1024)) and np.array_equal((m * HW).astype(np.float32).astype(F64), m * HW)
            assert np.abs(m * HW).max() < 2 ** 17                 # one pixel's g (>= 1/128 where non-zero) is at least one ulp
        for key in ("dx", "dskip", "dgamma", "dbeta", "dgamma2", "dbeta2"):
            if key in o:
                assert np.array_equal(o[key].astype(np.float32).astype(F64), o[key]), f"{key} is not exact in float32"
        outs.append(o)
    return outs


def eighths_case(N, H, W, C, seed=0):
    """Second exact family, for the forward sums alone: x = k/8, |k| <= 32.  x (granule 1/8, |x| <= 4) and x^2 (granule 1/64,
    <= 16) keep per-chunk sums exact in float32 up to 4096 pixels per chunk: 4096 * 16 * 64 = 2^22 granules."""
    return np.random.default_rng([22, N, H, W, C, seed]).integers(-32, 33, (N, H, W, C)).astype(F64) / 8.0


def eighths_premise(x, rpc):
    N, H, W, C = x.shape
    assert np.array_equal(x * 8, np.round(x * 8)) and np.abs(x).max() <= 4 and rpc <= 4096
    xs = x.reshape(N, H * W, C)
    for p0 in range(0, H * W, rpc):
        blk = xs[:, p0:p0 + rpc]
        for t in (blk, blk * blk):
            run32 = np.cumsum(t.astype(np.float32), axis=1, dtype=np.float32)
            assert np.array_equal(run32.astype(F64), np.cumsum(t, axis=1)), "float32 running sum differs from float64"


# ---------------------------------------------------------------------------- the random family
MARGIN = 64.0                                  # pre-activations stay this many forward bounds away from the kink


def random_case(name, N, H, W, C, act, leak, seed=0, pair=None, degenerate=False, one_launch=True):
    """Seeded normal data x * 1.5 + 0.3 rounded to the storage type, gamma = 1 + 0.2 n, beta = 0.2 n (float32), residual / skip /
    dy standard normal.  Elements whose oracle pre-activation (plain form: moved through x; skip form: through skip) lies within
    MARGIN forward bounds of 0 are moved away; nothing is excluded from any comparison.  degenerate: channels 0..2 of every image
    become a constant (0.5), a constant that float32 sums cannot hold exactly (1000.1) and a large mean over a small spread
    (50 +- 0.5); their beta is pushed out to where the margin holds for a constant pre-activation."""
    rng = np.random.default_rng([23, N, H, W, C, act, seed, int(degenerate), {"f32": 0, "bf16": 1}[name]])
    HW = H * W
    q = lambda a: to_storage(a, name)
    x = q(rng.standard_normal((N, H, W, C)) * 1.5 + 0.3)
    gamma = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32).astype(F64)
    beta = (0.2 * rng.standard_normal(C)).astype(np.float32).astype(F64)
    out = {"name": name, "eps": 1e-3, "leak": leak, "act": act, "pair": None, "planted": 0}
    if pair is not None:
        g2 = (-1.5 + 0.2 * rng.standard_normal(C)).astype(np.float32).astype(F64)      # visibly another set
        b2 = (0.7 + 0.2 * rng.standard_normal(C)).astype(np.float32).astype(F64)
        out.update(gamma2=g2, beta2=b2, pair=(g2, b2, pair))
    if degenerate:
        assert C >= 8 and pair is None
        out["planted"] = 3
        x[..., 0] = q(0.5)
        x[..., 1] = q(1000.1)
        x[..., 2] = q(50 + 0.5 * rng.standard_normal((N, H, W)))
        gamma[1] = 2.0 ** -6
        beta[:3] = (0.5, -0.5, 0.25)
    rel = sum_rel(name, chain_pixels(HW, one_launch))
    fb = lambda skip=None: forward_bounds(x, gamma, beta, out["eps"], act, leak, name, rel, None, skip, out["pair"])
    if act != NONE:
        for _ in range(50):
            pre, b = forward(x, gamma, beta, out["eps"], act, leak, pair=out["pair"])[3], fb()[1]
            near = np.abs(pre) < 2 * MARGIN * b
            if not near.any():
                break
            # constant channels (all of them at HW = 1) and the planted large-mean channel, whose bound is a sizeable fraction of
            # |gamma xhat|: the pre-activation is moved through beta, never through x
            fixed = set(np.flatnonzero((x.reshape(N, HW, C).var(1) == 0).any(0)).tolist()) | ({2} if degenerate else set())
            for c in sorted(fixed):
                if near[..., c].any():
                    reach = np.abs(pre[..., c] - beta[c]).max() + 4 * MARGIN * b[..., c].max()
                    beta[c] = np.float32((1 if beta[c] >= 0 else -1) * max(2 * abs(beta[c]), reach))
            near[..., sorted(fixed)] = False
            x[near] = q(x[near] + np.where(rng.integers(0, 2, int(near.sum())) == 0, 0.375, -0.375))
        else:
            raise AssertionError("kink margin not reached")
    skip = q(rng.standard_normal((N, H, W, C)))
    if act != NONE:
        for _ in range(50):
            pre = forward(x, gamma, beta, out["eps"], act, leak, skip=skip, pair=out["pair"])[3]
            near = np.abs(pre) < 2 * MARGIN * fb(skip)[1]
            if not near.any():
                break
            skip[near] = q(skip[near] + np.where(pre[near] >= 0, 0.375, -0.375))
        else:
            raise AssertionError("kink margin not reached (skip form)")
    out.update(x=x, gamma=gamma, beta=beta, skip=skip, residual=q(rng.standard_normal((N, H, W, C))),
               dy=q(rng.standard_normal((N, H, W, C))), dy32=rng.standard_normal((N, H, W, C)).astype(np.float32).astype(F64))
    out["dy_skip"] = out["dy"]
    return out


# ---------------------------------------------------------------------------- the cases both test files use
# (N, H, W, C per dtype, why).  Each is the smallest shape that reaches its edge.
ACT_GRID = ((NONE, 0.0), (RELU, 0.0), (LRELU, 0.2), (LRELU, 0.3))
SHAPES = (
    # one-launch path: a block walks the pixels in strides of 64 rows -> 1 pixel, one short of a stride, a stride, a stride + 1;
    # C = 8 / 40: 2 or 10 (f32), 1 or 5 (bf16) channel vectors, so the last block of 4 vectors is part dead
    ((2, 1, 1), {"f32": 8, "bf16": 8}), ((2, 1, 1), {"f32": 40, "bf16": 40}),
    ((2, 7, 9), {"f32": 8, "bf16": 8}), ((2, 7, 9), {"f32": 40, "bf16": 40}),
    ((2, 8, 8), {"f32": 8, "bf16": 8}), ((2, 8, 8), {"f32": 40, "bf16": 40}),
    ((2, 5, 13), {"f32": 8, "bf16": 8}), ((2, 5, 13), {"f32": 40, "bf16": 40}),
    # the switch: 512 pixels is the last one-launch map, 513 the first split one (9 chunks of 64, the last of 1 pixel; with
    # C = 8 the 128 (f32) / 256 (bf16) pixel rows in flight exceed the chunk length)
    ((2, 16, 32), {"f32": 8, "bf16": 8}), ((2, 16, 32), {"f32": 40, "bf16": 40}),
    ((2, 19, 27), {"f32": 8, "bf16": 8}), ((2, 19, 27), {"f32": 40, "bf16": 40}),
    # lanes that do not divide 256 (C = 40: 10 / 5 vectors) and lanes that do (C = 64: 16 / 8); 1320 pixels = 20 chunks of 64
    # + one of 40: the unrolled body and the one-pixel tail run in one block
    ((2, 19, 27), {"f32": 64, "bf16": 64}), ((2, 33, 40), {"f32": 40, "bf16": 40}), ((2, 33, 40), {"f32": 64, "bf16": 64}),
    # 8193 pixels: 128 pixels per chunk, 65 chunks, the last of 1 pixel
    ((1, 3, 2731), {"f32": 8, "bf16": 8}),
    # 133225 pixels: 65 pixels per apply block (2050 blocks, the last of 40 pixels), 1088 per chunk, 123 chunks
    ((1, 365, 365), {"f32": 8, "bf16": 8}),
    # more than 256 channel vectors: the second sweep over the channel vectors (258 / 257 vectors)
    ((1, 19, 27), {"f32": 1032, "bf16": 2056}),
)
BIG = (1, 3, 174763, 8)                        # 524289 pixels: 4096 per chunk, 129 chunks (second trip of the finalize reduction),
                                               # 256 pixels per apply block, 2049 blocks; f32, exact family only (17 MB)
CHUNK_COUNTS = (1, 31, 32, 33, 127, 128, 129, 300)      # caller-supplied statistics rows, at (2, 8, 8, 40)
CHUNK_SHAPE = (2, 8, 8, 40)
PAIR_SHAPES = ((2, 8, 8, 40, 1), (3, 8, 8, 40, 1), (3, 8, 8, 40, 2), (2, 19, 27, 40, 1), (3, 19, 27, 40, 1), (3, 19, 27, 40, 2))
DEGENERATE_SHAPES = ((2, 8, 8, 8), (2, 33, 40, 8))
KINK_SHAPES = ((2, 8, 8, 8), (2, 33, 40, 40))
SENTINEL_SHAPES = ((2, 8, 8, 40), (2, 19, 27, 40))       # one-launch and split; C_real = 34 of 40
C_REAL = 34


def all_specs():
    """Every case of tests/test_gpu_instnorm.py as a dict (group, id, family, name, N, H, W, C, act, leak, pair, ...); build(spec)
    makes its inputs.  tests/test_instnorm_oracle_cpu.py checks premise, margin and the reference emulation for each."""
    specs = []

    def add(group, family, name, N, H, W, C, act, leak, pair=None, **kw):
        leak = EXACT_LEAK if (family == "exact" and act == LRELU) else leak
        tag = f"{group}-{family}-{N}x{H}x{W}x{C}-{name}-act{act}" + (f"-ns{pair}" if pair else "")
        specs.append(dict(group=group, id=tag, family=family, name=name, N=N, H=H, W=W, C=C, act=act, leak=leak, pair=pair, **kw))

    for _, name, N, H, W, C, act, leak in shape_cases():
        for family in ("random", "exact"):
            add("shape", family, name, N, H, W, C, act, leak)
    add("big", "exact", "f32", *BIG, RELU, 0.0)
    for i, (N, H, W, C, ns) in enumerate(PAIR_SHAPES):
        for j, name in enumerate(("f32", "bf16")):
            for family in ("random", "exact"):
                add("pair", family, name, N, H, W, C, *ACT_GRID[(i + j + 1) % 4], pair=ns)
    for i, shp in enumerate(DEGENERATE_SHAPES):
        for name in ("f32", "bf16"):
            add("degenerate", "random", name, *shp, *((RELU, 0.0), (LRELU, 0.3))[i], degenerate=True)
    for shp in KINK_SHAPES:
        for name in ("f32", "bf16"):
            for act in (RELU, LRELU):
                add("kink", "exact", name, *shp, act, EXACT_LEAK, want_zeros=True)
    for shp in SENTINEL_SHAPES:
        for name in ("f32", "bf16"):
            for ns in (None, 1):
                add("sentinel", "exact", name, *shp, LRELU, EXACT_LEAK, pair=ns)
    for name in ("f32", "bf16"):
        for family in ("random", "exact"):
            add("chunks", family, name, *CHUNK_SHAPE, RELU, 0.0)
    return specs


def specs_of(group):
    return [s for s in all_specs() if s["group"] == group]


def build(spec):
    s = spec
    if s["family"] == "exact":
        return cached_exact(s["name"], s["N"], s["H"], s["W"], s["C"], s["act"], want_zeros=s.get("want_zeros", False), pair=s["pair"])
    return cached_random(s["name"], s["N"], s["H"], s["W"], s["C"], s["act"], s["leak"], pair=s["pair"], degenerate=s.get("degenerate", False))


def shape_cases():
    """(id, name, N, H, W, C, act, leak) of the per-shape grid: the activations are spread over it, not crossed with it."""
    out = []
    for i, ((N, H, W), Cs) in enumerate(SHAPES):
        for j, name in enumerate(("f32", "bf16")):
            act, leak = ACT_GRID[(i + 2 * j) % len(ACT_GRID)]
            out.append((f"{N}x{H}x{W}x{Cs[name]}-{name}", name, N, H, W, Cs[name], act, leak))
    return out


@functools.lru_cache(maxsize=8)
def cached_random(*a, **k):
    return random_case(*a, **k)


@functools.lru_cache(maxsize=8)
def cached_exact(*a, **k):
    return exact_case(*a, **k)
