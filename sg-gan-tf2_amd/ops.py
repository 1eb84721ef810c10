"""The reference's primitive vocabulary -- ``conv2d / deconv2d / instance_norm / lrelu`` (ops.py:13-37;
conv2d/deconv2d are commented out there at :24-34, the live layers are the Keras ones in module.py) --
as differentiable ops over the HIP kernels.  Numerics follow the LIVE path by default
(InstanceNorm eps=1e-3, LeakyReLU alpha=0.3); pass ``eps=1e-5`` / ``leak=0.2`` for the ops.py spec.

Tensors are NHWC on the GPU, float32 or bfloat16.  Channel counts that are not a multiple of 8 are
zero-padded on the way in and cropped on the way out (the kernels work on 16-byte channel chunks).
Weights use the reference layouts: HWIO for conv2d, (kh,kw,out,in) for deconv2d; parameters and their
gradients are float32.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _abi as A
from . import kernels as K


def _padc(x, cp):
    return x if x.shape[-1] == cp else F.pad(x, (0, cp - x.shape[-1]))


def _vec(v, cp):
    v = v.to(torch.float32)
    return (v if v.numel() == cp else F.pad(v, (0, cp - v.numel()))).contiguous()


def _parse_padding(padding):
    """'SAME' | 'VALID' | 'REFLECT-p' (tf.pad REFLECT of p, then VALID)."""
    if isinstance(padding, str) and padding.upper().startswith("REFLECT"):
        return "VALID", int(padding.split("-")[1])
    return padding.upper(), 0


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, padding, reflect, act, leak):
        R, S, Cr, Kr = w.shape
        Cp, Kp = K.cpad(Cr), K.cpad(Kr)
        xp = _padc(x, Cp).contiguous()
        N, H, W, _ = xp.shape
        g = K.conv_geom(N, H, W, Cp, Kp, R, S, stride, padding, reflect, xp.dtype)
        wf, wd = K.pack_weights(w.detach().to(torch.float32).contiguous(), Cp, Kp, xp.dtype)
        y = K.conv_fwd(g, xp, wf, None if b is None else _vec(b.detach(), Kp), act, leak)
        ctx.g, ctx.act, ctx.leak, ctx.dims, ctx.has_b = g, act, leak, (Cr, Kr, x.shape[-1]), b is not None
        ctx.save_for_backward(xp, wd, y)
        return y[..., :Kr] if Kp != Kr else y

    @staticmethod
    def backward(ctx, dy):
        xp, wd, y = ctx.saved_tensors
        Cr, Kr, Cx = ctx.dims
        g = ctx.g
        dy = _padc(dy.to(xp.dtype), g.y_shape[-1]).contiguous()
        if ctx.act != A.ACT_NONE:
            dy = K.act_bwd(dy, y, ctx.act, ctx.leak)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = K.conv_dgrad(g, dy, wd)[..., :Cx]
        if ctx.needs_input_grad[1]:
            dw = torch.empty((g.desc.R, g.desc.S, Cr, Kr), dtype=torch.float32, device=dy.device)
            K.conv_wgrad(g, xp, dy, dw)
        if ctx.has_b and ctx.needs_input_grad[2]:
            db = torch.empty(Kr, dtype=torch.float32, device=dy.device)
            K.bias_grad(dy, db)
        return dx, dw, db, None, None, None, None, None


class _Deconv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, act, leak):
        R, S, Co, Ci = w.shape
        Cop, Cip = K.cpad(Co), K.cpad(Ci)
        xp = _padc(x, Cip).contiguous()
        N, H, W, _ = xp.shape
        g = K.deconv_geom(N, H, W, Cip, Cop, R, S, stride, xp.dtype)
        wf, wd = K.pack_weights(w.detach().to(torch.float32).contiguous(), Cop, Cip, xp.dtype)
        y = K.deconv_fwd(g, xp, wd, None if b is None else _vec(b.detach(), Cop), act, leak)
        ctx.g, ctx.act, ctx.leak, ctx.dims, ctx.has_b = g, act, leak, (Co, Ci, x.shape[-1]), b is not None
        ctx.save_for_backward(xp, wf, y)
        return y[..., :Co] if Cop != Co else y

    @staticmethod
    def backward(ctx, dy):
        xp, wf, y = ctx.saved_tensors
        Co, Ci, Cx = ctx.dims
        g = ctx.g
        dy = _padc(dy.to(xp.dtype), g.y_shape[-1]).contiguous()
        if ctx.act != A.ACT_NONE:
            dy = K.act_bwd(dy, y, ctx.act, ctx.leak)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = K.deconv_dgrad(g, dy, wf)[..., :Cx]
        if ctx.needs_input_grad[1]:
            dw = torch.empty((g.desc.R, g.desc.S, Co, Ci), dtype=torch.float32, device=dy.device)
            K.deconv_wgrad(g, xp, dy, dw)
        if ctx.has_b and ctx.needs_input_grad[2]:
            db = torch.empty(Co, dtype=torch.float32, device=dy.device)
            K.bias_grad(dy, db)
        return dx, dw, db, None, None, None


class _InstanceNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, act, leak):
        Cr = x.shape[-1]
        Cp = K.cpad(Cr)
        xp = _padc(x, Cp).contiguous()
        g, b = _vec(gamma.detach(), Cp), _vec(beta.detach(), Cp)
        y, stats = K.instnorm_fwd(xp, g, b, None, eps, act, leak)
        ctx.act, ctx.leak, ctx.Cr = act, leak, Cr
        ctx.save_for_backward(xp, g, b, stats)
        return y[..., :Cr] if Cp != Cr else y

    @staticmethod
    def backward(ctx, dy):
        xp, g, b, stats = ctx.saved_tensors
        dy = _padc(dy.to(xp.dtype), xp.shape[-1]).contiguous()
        dg = torch.empty(ctx.Cr, dtype=torch.float32, device=dy.device)
        db = torch.empty(ctx.Cr, dtype=torch.float32, device=dy.device)
        dx = K.instnorm_bwd(dy, xp, g, b, stats, dg, db, False, ctx.act, ctx.leak)
        return dx[..., :ctx.Cr], dg, db, None, None, None


class _ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, leak):
        Cr = x.shape[-1]
        xp = _padc(x, K.cpad(Cr)).contiguous()
        y = K.act_fwd(xp, act, leak)
        ctx.act, ctx.leak, ctx.Cr = act, leak, Cr
        ctx.save_for_backward(y)
        return y[..., :Cr] if y.shape[-1] != Cr else y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _padc(dy.to(y.dtype), y.shape[-1]).contiguous()
        return K.act_bwd(dy, y, ctx.act, ctx.leak)[..., :ctx.Cr], None, None


class _DiffAugmentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params):
        Cr = x.shape[-1]
        xp = _padc(x, K.cpad(Cr)).contiguous()
        par = params.detach().to(torch.float32).contiguous()
        ctx.Cr = Cr
        ctx.save_for_backward(par)
        y = K.diffaug(xp, par, Cr)
        return y[..., :Cr] if y.shape[-1] != Cr else y

    @staticmethod
    def backward(ctx, dy):
        (par,) = ctx.saved_tensors
        dy = _padc(dy, K.cpad(ctx.Cr)).contiguous()
        return K.diffaug_bwd(dy, par, ctx.Cr)[..., :ctx.Cr], None


class _SsimLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, data_range):
        Cr = x.shape[-1]
        Cp = K.cpad(Cr)
        xp = _padc(x.detach().to(torch.float32), Cp).contiguous()
        tp = _padc(target.detach().to(torch.float32), Cp).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        dx = torch.empty_like(xp) if ctx.needs_input_grad[0] else None
        K.ssim_loss(tp, xp, Cr, loss, dx, data_range=data_range)     # the gradient is the forward's by-product: kept for backward
        ctx.Cr = Cr
        ctx.save_for_backward(dx)
        return loss[0]

    @staticmethod
    def backward(ctx, dl):
        (dx,) = ctx.saved_tensors
        return dx[..., :ctx.Cr] * dl, None, None


class _FeatureMatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, *tensors):
        fakes, reals = tensors[:n], tensors[n:]
        crs = [f.shape[-1] for f in fakes]
        fp = [_padc(f.detach().to(torch.float32), K.cpad(c)).contiguous() for f, c in zip(fakes, crs)]
        rp = [_padc(r.detach().to(torch.float32), K.cpad(c)).contiguous() for r, c in zip(reals, crs)]
        loss, term = (torch.empty(1, dtype=torch.float32, device=fp[0].device) for _ in range(2))
        grads = K.feature_match(rp, fp, crs, loss, term, 1.0)        # the gradients are the forward's by-product: kept for backward
        ctx.crs = crs
        ctx.save_for_backward(*grads)
        return term[0]

    @staticmethod
    def backward(ctx, dl):
        return (None,) + tuple(g[..., :c] * dl for g, c in zip(ctx.saved_tensors, ctx.crs)) + (None,) * len(ctx.crs)


class _Upsample2xFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode):
        Cr = x.shape[-1]
        xp = _padc(x.detach(), K.cpad(Cr)).contiguous()
        ctx.mode, ctx.Cr, ctx.dtype = mode, Cr, xp.dtype
        y = K.upsample2x(xp, mode)
        return y[..., :Cr] if y.shape[-1] != Cr else y

    @staticmethod
    def backward(ctx, dy):
        dy = _padc(dy.to(ctx.dtype), K.cpad(ctx.Cr)).contiguous()
        return K.upsample2x_bwd(dy, ctx.mode)[..., :ctx.Cr], None


_ACTS = {None: A.ACT_NONE, "none": A.ACT_NONE, "relu": A.ACT_RELU, "lrelu": A.ACT_LRELU, "tanh": A.ACT_TANH}


def conv2d(x, w, b=None, stride=1, padding="SAME", act=None, leak=0.3):
    """tf.keras.layers.Conv2D(k, (R,S), strides, padding) [+ tf.pad REFLECT via padding='REFLECT-p'] (module.py:210-311).
    TF 'SAME' is asymmetric (extra pad bottom/right)."""
    pad, reflect = _parse_padding(padding)
    return _Conv2dFn.apply(x, w, b, int(stride), pad, reflect, _ACTS[act], float(leak))


def deconv2d(x, w, b=None, stride=2, act=None, leak=0.3):
    """tf.keras.layers.Conv2DTranspose(k, (3,3), strides=(2,2), padding='same') (module.py:254,258); w is (kh,kw,out,in)."""
    return _Deconv2dFn.apply(x, w, b, int(stride), _ACTS[act], float(leak))


def instance_norm(x, gamma, beta, eps=1e-3, act=None, leak=0.3):
    """tfa.layers.InstanceNormalization (module.py:212..308); eps=1e-5 gives ops.instance_norm (ops.py:13-22)."""
    return _InstanceNormFn.apply(x, gamma, beta, float(eps), _ACTS[act], float(leak))


def lrelu(x, leak=0.3):
    """tf.keras.layers.LeakyReLU() alpha=0.3 (module.py:285-309); leak=0.2 gives ops.lrelu (ops.py:36-37)."""
    return _ActFn.apply(x, A.ACT_LRELU, float(leak))


def relu(x):
    return _ActFn.apply(x, A.ACT_RELU, 0.0)


def tanh(x):
    return _ActFn.apply(x, A.ACT_TANH, 0.0)


def diff_augment(x, params):
    """Differentiable augmentation in front of a discriminator (Zhao et al. 2020, colour + cutout): x (N,H,W,C)
    with C <= 8, params (N,8) f32 rows [b, s, c, y0, x0, ch, cw, 0] (kernels.diffaug_draw fills them on the device).  The
    transform is affine in x for fixed rows; the gradient w.r.t. x is its adjoint, params get none."""
    return _DiffAugmentFn.apply(x, params)


def ssim_loss(x, target, data_range=1.0):
    """1 - mean SSIM(target, x) as a scalar (Wang et al.'s index, 11 x 11 Gaussian window of sigma 1.5, the windows
    wholly inside the image): x, target (N,H,W,C) float32 with C <= 8 and H, W >= 11, values spanning ``data_range``.  target is
    a constant; the gradient w.r.t. x is the kernel's closed form (sgg_ssim_loss)."""
    if x.shape != target.shape or x.dim() != 4 or x.shape[-1] > A.CPAD:
        raise ValueError(f"ssim_loss: x {tuple(x.shape)} and target {tuple(target.shape)} must be equal (N,H,W,C) with C <= {A.CPAD}")
    return _SsimLossFn.apply(x, target, float(data_range))


def feature_match(fakes, reals):
    """The feature-matching term (Wang et al. 2018) as a scalar: the mean over the pairs of mean |fake_i - real_i|,
    for 1 to 8 pairs of (..., C_i) float32 tensors of equal shapes.  The reals are constants; the gradient goes to ``fakes`` only
    (sign(fake - real) / (L * numel_i), 0 where they are equal), computed by the same call (sgg_feature_match)."""
    fakes, reals = list(fakes), list(reals)
    if not 1 <= len(fakes) <= A.FM_MAX_PAIRS or len(reals) != len(fakes) or any(f.shape != r.shape or f.dim() < 2 for f, r in zip(fakes, reals)):
        raise ValueError(f"feature_match: 1..{A.FM_MAX_PAIRS} pairs of equally shaped (..., C) tensors, got "
                         f"{[tuple(f.shape) for f in fakes]} against {[tuple(r.shape) for r in reals]}")
    return _FeatureMatchFn.apply(len(fakes), *fakes, *reals)


def upsample2x(x, mode="nearest"):
    """The fixed 2x resampling of the resize-convolution layers: x (N,H,W,C) float32 or bfloat16 -> (N,2H,2W,C).
    mode 'nearest' (tf.keras.layers.UpSampling2D()) or 'bilinear' (half-pixel centres: UpSampling2D(interpolation="bilinear"),
    torch's align_corners=False).  The gradient w.r.t. x is the adjoint of the same linear map (sgg_upsample2x_bwd)."""
    K.upsample_mode(mode)
    if x.dim() != 4:
        raise ValueError(f"upsample2x: x {tuple(x.shape)} must be (N,H,W,C)")
    return _Upsample2xFn.apply(x, mode)
