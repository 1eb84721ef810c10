"""NumPy / torch statement of the U-Net decoder's training-mode dropout, test infrastructure only:

  * Philox4x32-10 vectorised over counter word 3 (checked against ``tests.diffaug_oracle.philox4x32_10``), the 16-bit draws and
    ``keep_mask`` -- integers only, so the device mask can be compared bit for bit;
  * ``apply``: the exact f32 / bf16 result of ``sgg_dropout`` (one f32 product, one rounding to the storage type, +0 where dropped);
  * ``torch_generator_unet``: ``tests.unet_oracle.torch_generator_unet`` in float64 with the three masks between the transposed
    conv and the instance norm of d1..d3 (``deconv -> mask * scale -> IN -> add``).
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import unet_oracle as U

F32, F64 = np.float32, np.float64
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, key):
    """Four counter words (scalars or arrays that broadcast), key (k0, k1) -> four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, np.uint64) & _LO for c in (c0, c1, c2, c3)))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(rate):
    """round(rate * 65536) clamped to 0..65535."""
    return min(max(int(round(float(rate) * 65536.0)), 0), 65535)


def scale(thr):
    """65536.f / (65536 - threshold), one f32 division."""
    return F32(65536.0) / F32(65536 - int(thr))


def draws(t, seed, stream_id, g, vecs):
    """The 16-bit draws of the first ``vecs`` vectors of global sample g: (vecs * 8,) uint32, element i = vector i / 8, lane i % 8."""
    t = int(t) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10(t & 0xFFFFFFFF, t >> 32, int(g) & 0xFFFFFFFF, np.arange(vecs, dtype=np.uint64), (seed, 1 + int(stream_id)))
    w = np.stack(r, -1)                                              # (vecs, 4)
    return np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], -1).reshape(-1)     # lane j: word j >> 1, half j & 1


def keep_mask(t, seed, stream_id, sample_offset, n, elems, rate):
    """(n, elems) bool: element i of row r (global sample sample_offset + r) is kept iff its draw >= threshold(rate)."""
    assert elems % 8 == 0
    thr = np.uint32(threshold(rate))
    return np.stack([draws(t, seed, stream_id, int(sample_offset) + r, elems // 8) >= thr for r in range(n)]) if n else np.zeros((0, elems), bool)


def layer_mask(t, seed, stream_id, sample_offset, n, H, W, C, rate):
    """keep_mask of an internal (n, H, W, cpad(C)) activation, cut to its C real channels: (n, H, W, C) bool."""
    Cp = (C + 7) // 8 * 8
    return keep_mask(t, seed, stream_id, sample_offset, n, H * W * Cp, rate).reshape(n, H, W, Cp)[..., :C]


def apply(x, mask, rate, bf16=False):
    """The kernel's result on x (float32 values; bf16=True: values a bf16 holds, and the result is rounded to bf16, returned as
    float32): kept elements x * scale formed in f32, dropped ones +0.  Rate 0 returns x's bits."""
    x = np.asarray(x, F32)
    thr = threshold(rate)
    if thr == 0:
        return x.copy()
    prod = (x * scale(thr)).astype(F32)
    if bf16:
        prod = torch.from_numpy(prod).to(torch.bfloat16).to(torch.float32).numpy()
    return np.where(mask.reshape(x.shape), prod, F32(0.0))


def masked_deconv_norm(h, w, b, gamma, beta, mask, s, eps=1e-3):
    """float64 torch: IN(mask * s * conv_transpose(h, w, b)), NCHW; w in the reference layout (kh, kw, out, in); mask None: no mask."""
    z = F.conv_transpose2d(h, w.permute(3, 2, 0, 1), b, padding=1)
    if mask is not None:
        z = z * mask * s
    return U._inorm(z, gamma, beta, eps)


class Kinks:
    """The activations' branch decisions of a kink-aware evaluation (the rule of oracle.sggan_oracle.KinkPolicy): the oracle's
    own sign, except within ``band`` of the kink, where the kernel's recorded decision (``branches``, NCHW bool tensors in
    evaluation order: e1..e8, d3, d7) is taken.  ``disagree_outside`` counts decisions that differ outside the band."""

    def __init__(self, branches, band=1e-4):
        self.branches, self.band, self.calls, self.ambiguous, self.disagree_outside = list(branches), band, 0, 0, 0

    def act(self, pre, leak):
        mine = pre.detach() > 0
        theirs = self.branches[self.calls]
        self.calls += 1
        near = pre.detach().abs() < self.band
        self.ambiguous += int(near.sum())
        self.disagree_outside += int(((mine != theirs) & ~near).sum())
        pos = torch.where(near, theirs, mine)
        return pre * torch.where(pos, 1.0, leak).to(pre.dtype)


def _act(pre, leak, kinks):
    return F.leaky_relu(pre, leak) if kinks is None else kinks.act(pre, leak)


def torch_generator_unet(P, x, masks, rate, eps=1e-3, kinks=None):
    """tests.unet_oracle.torch_generator_unet with ``masks`` = the (N, C, H, W) float64 0 / 1 tensors of d1, d2, d3.
    kinks: a Kinks holding the kernel's branch decisions (None: the oracle's own)."""
    s = float(scale(threshold(rate)))
    conv = lambda h, n: F.conv2d(h, P[n + "_w"].permute(3, 2, 0, 1), P[n + "_b"], padding=1)
    e, h = [], x
    for i in range(1, 8):
        h = _act(U._inorm(conv(h, f"e{i}"), P[f"e{i}_g"], P[f"e{i}_beta"], eps), U.LEAK, kinks)
        e.append(h)
    h = _act(U._inorm(conv(h, "e8"), P["e8_g"], P["e8_beta"], eps), 0.0, kinks)
    for i in range(1, 8):
        n = f"d{i}"
        h = masked_deconv_norm(h, P[n + "_w"], P[n + "_b"], P[n + "_g"], P[n + "_beta"], masks[i - 1] if i <= 3 else None, s, eps) + e[7 - i]
        if i in U.RELU_AFTER_ADD:
            h = _act(h, 0.0, kinks)
    return torch.tanh(F.conv_transpose2d(h, P["d8_w"].permute(3, 2, 0, 1), P["d8_b"], padding=1))


def nchw_masks(t, seed, application, sample_offset, n, H, W, C, rate):
    """The float64 NCHW masks of d1..d3 (all three are (n, H, W, C)) for one application of a generator at step t."""
    return [torch.from_numpy(layer_mask(t, seed, 4 * application + l, sample_offset, n, H, W, C, rate).astype(F64)).permute(0, 3, 1, 2)
            for l in range(3)]
