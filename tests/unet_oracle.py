"""Float64 oracle of generator_unet (reference module.py:125-206) and of the reference-mode train step with it as the
generator (model.py:169-200) -- TEST INFRASTRUCTURE ONLY, composed from the primitives of ``oracle/sggan_oracle.py``.

Two independent statements of the same network:
* ``generator_unet`` / ``train_step``: the NumPy float64 tape of ``oracle.sggan_oracle`` (Conv2D SAME, Conv2DTranspose
  stride 1, instance norm, LeakyReLU 0.3, ReLU, tanh, add), kink-aware through ``oracle.sggan_oracle.KINKS``;
* ``torch_generator_unet``: float64 torch autograd over ``F.conv2d`` / ``F.conv_transpose2d`` (NCHW).

Semantics pinned here (DESIGN.md "U-Net generator"): every conv is 3x3 stride 1 'same' with a bias; IN is tfa's (eps 1e-3,
gamma / beta); LeakyReLU() is Keras' default alpha 0.3; Dropout is the identity (the reference calls the generator without
``training=``, so Keras runs it in inference mode) [3P-recall]; d3 and d7 apply ReLU AFTER the skip add, d1, d2, d4-d6 have no
activation; d8 has no norm and ends in tanh.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sggan_oracle as O

LEAK = 0.3
RELU_AFTER_ADD = (3, 7)


def unet_param_shapes(gf_dim=64, in_c=3, out_c=3):
    """(name, shape) in Keras creation order: per layer kernel, bias, then IN gamma, beta; d8 has no norm.
    Conv2D kernels HWIO, Conv2DTranspose kernels (kh, kw, out, in)."""
    L = []

    def layer(name, shape, norm=True):
        out = shape[3] if name.startswith("e") else shape[2]
        L.extend([(name + "_w", shape), (name + "_b", (out,))])
        if norm:
            L.extend([(name + "_g", (out,)), (name + "_beta", (out,))])

    enc = [in_c, gf_dim, gf_dim * 2, gf_dim * 4] + [gf_dim * 8] * 5
    for i in range(1, 9):
        layer(f"e{i}", (3, 3, enc[i - 1], enc[i]))
    dec = [gf_dim * 8] * 5 + [gf_dim * 4, gf_dim * 2, gf_dim]
    for i in range(1, 8):
        layer(f"d{i}", (3, 3, dec[i], dec[i - 1]))
    layer("d8", (3, 3, out_c, gf_dim), norm=False)
    return L


def generator_unet(tape, P, x, eps=1e-3, leak=LEAK):
    """module.py:125-206 on the oracle tape.  P: name -> Var; x: Var (N,H,W,C)."""
    def cin(name, h, deconv):
        f = (lambda: O.deconv2d(tape, h, P[name + "_w"], P[name + "_b"], stride=1)) if deconv else \
            (lambda: O.conv2d(tape, h, P[name + "_w"], P[name + "_b"], 1, "SAME"))
        return O.instance_norm(tape, f(), P[name + "_g"], P[name + "_beta"], eps)

    e, h = [], x
    for i in range(1, 8):                                           # :139-165
        h = O.lrelu(tape, cin(f"e{i}", h, False), leak)
        e.append(h)
    h = O.relu(tape, cin("e8", h, False))                           # :167-169
    for i in range(1, 8):                                           # :171-202 (Dropout: identity)
        h = O.add(tape, cin(f"d{i}", h, True), e[7 - i])
        if i in RELU_AFTER_ADD:
            h = O.relu(tape, h)
    h = O.deconv2d(tape, h, P["d8_w"], P["d8_b"], stride=1)         # :204
    return O.tanh(tape, h)                                          # :205


def train_step(PG, PD, real_A, seg_A, mask_A, opt_state=None, t=1, lr=1e-3, beta1=0.5, leak=0.3, eps=1e-3, l1_lambda=100.0):
    """oracle.sggan_oracle.train_step with generator_unet as the generator (model.py:169-200, deviation D2); same returns."""
    tape = O.Tape()
    VG = {k: O.Var(v, k) for k, v in PG.items()}
    VD = {k: O.Var(v, k) for k, v in PD.items()}
    xA = O.Var(real_A)
    fake = generator_unet(tape, VG, xA, eps, LEAK)                      # :175-179
    seg = O.Var(seg_A)
    da_real = O.discriminator(tape, VD, seg, mask_A, leak, eps)         # :186
    da_fake = O.discriminator(tape, VD, fake, mask_A, leak, eps)        # :187 (=:188)
    gan = O.bce_logits_mean(tape, da_fake, 1.0)                         # :153
    l1 = O.l1_mean(tape, np.asarray(seg_A, O.F64), fake)                # :155
    gen_loss = O.scale_add(tape, gan, l1, l1_lambda)                    # :156
    real_l = O.bce_logits_mean(tape, da_real, 1.0)                      # :162
    fake_l = O.bce_logits_mean(tape, da_fake, 0.0)                      # :163
    disc_loss = O.scale_add(tape, real_l, fake_l, 1.0)                  # :164

    def grads(loss, wrt):
        for v in [xA, seg] + list(VG.values()) + list(VD.values()) + [o for o, _ in tape.ops]:
            v.g = None
        tape.backward([(loss, 1.0)])
        return {k: (np.zeros_like(v.v) if v.g is None else v.g.copy()) for k, v in wrt.items()}

    gG = grads(gen_loss, VG)
    gD = grads(disc_loss, VD)
    if opt_state is None:
        opt_state = {s: {k: np.zeros_like(v) for k, v in P.items()} for s, P in (("mG", PG), ("vG", PG), ("mD", PD), ("vD", PD))}
    newG, newD, st = {}, {}, {"mG": {}, "vG": {}, "mD": {}, "vD": {}}
    for k in PG:                                                        # :199
        newG[k], st["mG"][k], st["vG"][k] = O.adam_tf(PG[k], gG[k], opt_state["mG"][k], opt_state["vG"][k], t, lr, beta1)
    for k in PD:                                                        # :200
        newD[k], st["mD"][k], st["vD"][k] = O.adam_tf(PD[k], gD[k], opt_state["mD"][k], opt_state["vD"][k], t, lr, beta1)
    return {"fake_A": fake.v, "da_real": da_real.v, "da_fake": da_fake.v,
            "gen_loss": float(gen_loss.v), "disc_loss": float(disc_loss.v),
            "gG": gG, "gD": gD, "PG": newG, "PD": newD, "opt_state": st}


def generator_forward_backward(PG, x, dy, eps=1e-3):
    """The oracle generator alone: (output, {name: dL/dparam}, dL/dx) for L = sum(output * dy)."""
    tape = O.Tape()
    VG = {k: O.Var(v, k) for k, v in PG.items()}
    vx = O.Var(x)
    y = generator_unet(tape, VG, vx, eps)
    tape.backward([(y, np.asarray(dy, O.F64))])
    return y.v, {k: v.g for k, v in VG.items()}, vx.g


# ----------------------------------------------------------------------------- independent torch float64 statement
def _inorm(x, g, b, eps):
    var, mu = torch.var_mean(x, dim=(2, 3), unbiased=False, keepdim=True)
    return (x - mu) * torch.rsqrt(var + eps) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def torch_generator_unet(P, x, eps=1e-3):
    """P: name -> float64 tensor in the reference layouts; x NCHW.  3x3 stride-1 'same' = padding 1 on both sides, for the
    conv and for the transposed conv (whose torch weight is (in, out, kh, kw))."""
    conv = lambda h, n: F.conv2d(h, P[n + "_w"].permute(3, 2, 0, 1), P[n + "_b"], padding=1)
    deconv = lambda h, n: F.conv_transpose2d(h, P[n + "_w"].permute(3, 2, 0, 1), P[n + "_b"], padding=1)
    e, h = [], x
    for i in range(1, 8):
        h = F.leaky_relu(_inorm(conv(h, f"e{i}"), P[f"e{i}_g"], P[f"e{i}_beta"], eps), LEAK)
        e.append(h)
    h = F.relu(_inorm(conv(h, "e8"), P["e8_g"], P["e8_beta"], eps))
    for i in range(1, 8):
        h = _inorm(deconv(h, f"d{i}"), P[f"d{i}_g"], P[f"d{i}_beta"], eps) + e[7 - i]
        if i in RELU_AFTER_ADD:
            h = F.relu(h)
    return torch.tanh(deconv(h, "d8"))


def torch_forward_backward(PG, x, dy, eps=1e-3):
    """Same contract as generator_forward_backward (NHWC arrays in and out)."""
    P = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in PG.items()}
    xt = torch.tensor(np.asarray(x), dtype=torch.float64).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = torch_generator_unet(P, xt, eps)
    (y * torch.tensor(np.asarray(dy), dtype=torch.float64).permute(0, 3, 1, 2)).sum().backward()
    return (y.detach().permute(0, 2, 3, 1).numpy(), {k: v.grad.numpy() for k, v in P.items()},
            xt.grad.permute(0, 2, 3, 1).numpy())


# ----------------------------------------------------------------------------- kink decisions of the HIP path
def unet_branches(G, tape, sl=slice(None)):
    """GeneratorUNet.forward records -> one boolean array per ReLU / LeakyReLU in the order generator_unet evaluates them
    (e1..e8, d3, d7): a layer's output is positive exactly where the kernel took the positive branch."""
    pos = lambda t, c: (t[sl][..., :c] > 0).cpu().numpy()
    out = [pos(tape[k + 1][1], G.enc[k].cout) for k in range(8)]      # e(k+1)'s output = the next layer's saved input
    out += [pos(tape[8 + i - 1][4], G.dec[i - 1].cout) for i in RELU_AFTER_ADD]   # d3 / d7: the skip unit keeps its output
    return out
