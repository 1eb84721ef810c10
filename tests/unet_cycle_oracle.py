"""Float64 oracle of the 2G+2D cycle step with generator_unet as both generators -- TEST INFRASTRUCTURE ONLY.

``cycle_step`` is ``oracle.sggan_oracle.cycle_step`` restated with ``tests.unet_oracle.generator_unet`` in place of
``generator_resnet``: the same Tape, the same criteria (mse_const_mean / bce_logits_mean, l1_mean, gradloss on seg_edge_weight,
add_scalars) and the same adam_tf, in the same order of evaluation.  ``torch_cycle_step`` is an independent float64 torch
autograd statement of the same step (tests.unet_oracle.torch_generator_unet + oracle/torch_restatement.py's discriminator and
criteria).  ``unet_cycle_step_branches`` reads, from a model's saved forward records, which side of every ReLU / LeakyReLU the
kernels took, in the order ``cycle_step`` evaluates them (the ``branches`` of oracle.sggan_oracle.KinkPolicy).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import sggan_oracle as O
from oracle import torch_restatement as T
from tests import unet_oracle as U
from tests.kink_helpers import discriminator_branches

NETS = ("Gab", "Gba", "Da", "Db")


def cycle_step(PGab, PGba, PDa, PDb, real_A, real_B, seg_A, seg_B, mask_A, mask_B, opt_state=None, t=1,
               lr=2e-4, beta1=0.5, L1_lambda=10.0, Lg_lambda=5.0, use_lsgan=True, leak=0.3, eps=1e-3):
    """oracle.sggan_oracle.cycle_step with the U-Net generators; same returns."""
    tape = O.Tape()
    V = lambda P: {k: O.Var(v, k) for k, v in P.items()}
    Gab, Gba, Da, Db = V(PGab), V(PGba), V(PDa), V(PDb)
    xA, xB = O.Var(real_A), O.Var(real_B)
    fake_B = U.generator_unet(tape, Gab, xA, eps)
    cyc_A = U.generator_unet(tape, Gba, fake_B, eps)
    fake_A = U.generator_unet(tape, Gba, xB, eps)
    cyc_B = U.generator_unet(tape, Gab, fake_A, eps)
    DB_fake = O.discriminator(tape, Db, fake_B, mask_A, leak, eps)
    DA_fake = O.discriminator(tape, Da, fake_A, mask_B, leak, eps)
    DA_real = O.discriminator(tape, Da, xA, mask_A, leak, eps)
    DB_real = O.discriminator(tape, Db, xB, mask_B, leak, eps)
    crit = (lambda x, z: O.mse_const_mean(tape, x, z)) if use_lsgan else (lambda x, z: O.bce_logits_mean(tape, x, z))
    wA, wB = O.seg_edge_weight(seg_A), O.seg_edge_weight(seg_B)
    g_loss = O.add_scalars(tape, [
        (1.0, crit(DA_fake, 1.0)), (1.0, crit(DB_fake, 1.0)),
        (L1_lambda, O.l1_mean(tape, np.asarray(real_A, O.F64), cyc_A)), (L1_lambda, O.l1_mean(tape, np.asarray(real_B, O.F64), cyc_B)),
        (Lg_lambda, O.gradloss(tape, fake_A, real_B, wB)), (Lg_lambda, O.gradloss(tape, fake_B, real_A, wA))])
    d_loss = O.add_scalars(tape, [(0.5, crit(DA_real, 1.0)), (0.5, crit(DA_fake, 0.0)),
                                  (0.5, crit(DB_real, 1.0)), (0.5, crit(DB_fake, 0.0))])
    nets = {"Gab": Gab, "Gba": Gba, "Da": Da, "Db": Db}

    def grads(loss, which):
        for v in [xA, xB] + [p for n in nets.values() for p in n.values()] + [o for o, _ in tape.ops]:
            v.g = None
        tape.backward([(loss, 1.0)])
        return {n: {k: (np.zeros_like(v.v) if v.g is None else v.g.copy()) for k, v in nets[n].items()} for n in which}

    G = grads(g_loss, ("Gab", "Gba"))
    G.update(grads(d_loss, ("Da", "Db")))
    params = {"Gab": PGab, "Gba": PGba, "Da": PDa, "Db": PDb}
    if opt_state is None:
        opt_state = {n: {"m": {k: np.zeros_like(v) for k, v in P.items()}, "v": {k: np.zeros_like(v) for k, v in P.items()}}
                     for n, P in params.items()}
    new, st = {}, {}
    for n, P in params.items():
        new[n], st[n] = {}, {"m": {}, "v": {}}
        for k in P:
            new[n][k], st[n]["m"][k], st[n]["v"][k] = O.adam_tf(P[k], G[n][k], opt_state[n]["m"][k], opt_state[n]["v"][k], t, lr, beta1)
    return {"fake_A": fake_A.v, "fake_B": fake_B.v, "cyc_A": cyc_A.v, "cyc_B": cyc_B.v, "g_loss": float(g_loss.v),
            "d_loss": float(d_loss.v), "grads": G, "params": new, "opt_state": st}


def unet_cycle_step_branches(m):
    """Activation decisions of one U-Net cycle step (``sggan(use_resnet=False, cycle=True, keep_tapes=True).tapes``) in the order
    ``cycle_step`` evaluates them: G_ab(real_A), G_ba(fake_B), G_ba(real_B), G_ab(fake_A), then the discriminators as
    tests.kink_helpers.cycle_step_branches orders them.  The paired step stacks [first network's images; second network's]:
    G_first = (G_ab(real_A); G_ba(real_B)), G_second = (G_ba(fake_B); G_ab(fake_A))."""
    t, n = m.tapes, m.tapes["n"]
    lo, hi = slice(0, n), slice(n, 2 * n)
    Gab, Gba, Da, Db = m.generator, m.generator_BA, m.discriminator, m.discriminator_B
    out = (U.unet_branches(Gab, t["G_first"], lo) + U.unet_branches(Gba, t["G_second"], lo)
           + U.unet_branches(Gba, t["G_first"], hi) + U.unet_branches(Gab, t["G_second"], hi))
    q = t.get("D_quad")
    if q is not None:
        out += (discriminator_branches(Db, q, slice(n, 2 * n)) + discriminator_branches(Da, q, slice(2 * n, 3 * n))
                + discriminator_branches(Da, q, slice(3 * n, 4 * n)) + discriminator_branches(Db, q, slice(0, n)))
    else:
        out += (discriminator_branches(Db, t["D_fake"], lo) + discriminator_branches(Da, t["D_fake"], hi)
                + discriminator_branches(Da, t["D_real"], lo) + discriminator_branches(Db, t["D_real"], hi))
    return out


# ----------------------------------------------------------------------------- independent torch float64 statement
def torch_cycle_step(P, real_A, real_B, seg_A, seg_B, mask_A, mask_B, L1_lambda=10.0, Lg_lambda=5.0, use_lsgan=True):
    """The same step under torch float64 autograd (NHWC arrays in): {"g_loss", "d_loss", "grads": {net: {name: array}}, images}.
    P: {"Gab" | "Gba" | "Da" | "Db": name -> array}."""
    import torch.nn.functional as F
    to = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64).permute(0, 3, 1, 2).contiguous()
    rA, rB, sA, sB, mA, mB = map(to, (real_A, real_B, seg_A, seg_B, mask_A, mask_B))
    Pt = {n: {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in P[n].items()} for n in NETS}
    fake_B = U.torch_generator_unet(Pt["Gab"], rA); cyc_A = U.torch_generator_unet(Pt["Gba"], fake_B)
    fake_A = U.torch_generator_unet(Pt["Gba"], rB); cyc_B = U.torch_generator_unet(Pt["Gab"], fake_A)
    DB_fake = T.discriminator(Pt["Db"], fake_B, mA); DA_fake = T.discriminator(Pt["Da"], fake_A, mB)
    DA_real = T.discriminator(Pt["Da"], rA, mA); DB_real = T.discriminator(Pt["Db"], rB, mB)
    if use_lsgan:
        crit = lambda x, z: ((x - z) ** 2).mean()
    else:
        crit = lambda x, z: F.binary_cross_entropy_with_logits(x, torch.full_like(x, z))
    wA, wB = T.seg_edge_weight(sA), T.seg_edge_weight(sB)
    g_loss = (crit(DA_fake, 1.0) + crit(DB_fake, 1.0) + L1_lambda * ((rA - cyc_A).abs().mean() + (rB - cyc_B).abs().mean())
              + Lg_lambda * (T.gradloss(fake_A, rB, wB) + T.gradloss(fake_B, rA, wA)))
    d_loss = 0.5 * (crit(DA_real, 1.0) + crit(DA_fake, 0.0)) + 0.5 * (crit(DB_real, 1.0) + crit(DB_fake, 0.0))
    grads = {}
    for loss, which, keep in ((g_loss, ("Gab", "Gba"), True), (d_loss, ("Da", "Db"), False)):
        ps = [p for n in which for p in Pt[n].values()]
        gs = iter(torch.autograd.grad(loss, ps, retain_graph=keep, allow_unused=True))
        for n in which:
            grads[n] = {k: (np.zeros(tuple(p.shape)) if (g := next(gs)) is None else g.numpy()) for k, p in Pt[n].items()}
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).numpy()
    return {"g_loss": g_loss.item(), "d_loss": d_loss.item(), "grads": grads, "fake_A": nhwc(fake_A), "fake_B": nhwc(fake_B),
            "cyc_A": nhwc(cyc_A), "cyc_B": nhwc(cyc_B)}
