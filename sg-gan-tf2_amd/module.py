"""Network definitions of the SG-GAN hot path -- host-side mirror of the reference's ``module.py``.

``generator_resnet()`` (module.py:219-269, with ``residule_block`` :208-217) and
``discriminator()`` (module.py:272-318) keep the reference's names and call
conventions (``generator(x)``, ``discriminator([x, mask])``) but run on an explicit
forward/backward engine over the HIP kernels of libsggan.so: no tracing compiler, no
autograd graph in the training loop.  Each network owns ONE flat f32 buffer for its
parameters, one for gradients and two for the Adam slots, so the optimizer is a single
launch and data-parallel training all-reduces one bucket per network.

Deviation D3: ``gf_dim/df_dim/segment_class`` and the image size are
parameters (defaults = the module-local constants of the reference); layers are
shape-agnostic, geometry is resolved per call.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _abi as A
from . import kernels as K


# ----------------------------------------------------------------------------- parameters
class ParamStore:
    """Flat parameter storage.  1-D parameters (bias, gamma, beta) are stored padded to the
    channel granule (8) so kernels can index them by padded channel; padded entries stay 0."""

    def __init__(self, specs, device):
        self.specs = list(specs)
        self.index = {}
        off = 0
        for name, shape in self.specs:
            shape = tuple(int(s) for s in shape)
            n = K.cpad(shape[0]) if len(shape) == 1 else int(np.prod(shape))
            self.index[name] = (off, n, shape)
            off += (n + 3) // 4 * 4
        self.numel = off
        self.device = torch.device(device)
        z = lambda: torch.zeros(self.numel, dtype=torch.float32, device=self.device)
        self.flat, self.grad, self.m, self.v = z(), z(), z(), z()
        self.version = 0            # bumped whenever parameter values change (re-pack trigger)
        self.loaded = 0             # bumped whenever the values are replaced wholesale (init, load): derived state starts over
        # Adam's step number lives on the device (Keras: the `optimizer.iterations` variable), so the update launch
        # carries no host state and can be replayed from a captured HIP graph
        self._adam_state = torch.zeros(2, dtype=torch.int64, device=self.device)    # [iterations, scratch] (sgg_adam_iter)
        self.iterations = self._adam_state[0:1]
        # the guarded update's record [last_norm, last_clip, skipped_total, applied_total] and workspace: device memory,
        # allocated at the first guarded step (guard_buffers), so a model without the options carries neither
        self._guard = self._guard_ws = None
        # the moving average of `flat` and its [d_t, 1 - d_t] (enable_ema): a store without it carries neither
        self.ema = self._ema_state = None

    @property
    def step_count(self):
        """Adam t (host copy of the device counter; synchronises -- checkpoint / test use only)."""
        return int(self.iterations.item())

    @step_count.setter
    def step_count(self, t):
        self.iterations.fill_(int(t))

    # views ------------------------------------------------------------------
    def _view(self, buf, name, padded):
        off, n, shape = self.index[name]
        if len(shape) == 1:
            return buf[off:off + n] if padded else buf[off:off + shape[0]]
        return buf[off:off + n].view(shape)

    def p(self, name, padded=True):
        return self._view(self.flat, name, padded)

    def g(self, name, padded=False, buf=None):
        return self._view(self.grad if buf is None else buf, name, padded)

    def names(self):
        return [n for n, _ in self.specs]

    def n_real(self):
        return sum(int(np.prod(s)) for _, s in self.specs)

    # init / io ----------------------------------------------------------------
    def init_keras(self, seed):
        """Keras defaults: glorot_uniform kernels, zero bias, IN gamma=1 / beta=0."""
        gen = torch.Generator(device="cpu").manual_seed(int(seed))
        host = torch.zeros(self.numel, dtype=torch.float32)
        for name, shape in self.specs:
            off, n, shape = self.index[name]
            if name.endswith("_w"):
                rf = int(np.prod(shape[:-2]))
                lim = math.sqrt(6.0 / (shape[-2] * rf + shape[-1] * rf))
                host[off:off + n] = (torch.rand(n, generator=gen) * 2 - 1) * lim
            elif name.endswith("_g"):
                host[off:off + shape[0]] = 1.0
        self.flat.copy_(host)
        self.version += 1
        self.loaded += 1

    def load(self, params: dict):
        """name -> array in the reference layouts (HWIO kernels, (kh,kw,out,in) transpose kernels)."""
        host = torch.zeros(self.numel, dtype=torch.float32)
        for name, _ in self.specs:
            off, n, shape = self.index[name]
            a = torch.as_tensor(np.asarray(params[name], dtype=np.float32)).reshape(-1)
            assert a.numel() == int(np.prod(shape)), (name, a.numel(), shape)
            host[off:off + a.numel()] = a
        self.flat.copy_(host)
        self.version += 1
        self.loaded += 1

    def export(self, buf=None) -> dict:
        src = (self.flat if buf is None else buf).detach().cpu()
        out = {}
        for name, _ in self.specs:
            off, n, shape = self.index[name]
            out[name] = src[off:off + int(np.prod(shape))].view(shape).numpy().copy()
        return out

    def zero_grad(self):
        self.grad.zero_()

    def guard_buffers(self):
        """(record, workspace) of the guarded update, allocated on first use -- before a step is captured: the recording's
        eager warm-up step gets here first."""
        if self._guard is None:
            self._guard = torch.zeros(4, dtype=torch.float64, device=self.device)
            self._guard_ws = K.grad_guard_workspace(self.numel, self.device)
        return self._guard, self._guard_ws

    def enable_ema(self):
        """Allocate ``ema``, the exponential moving average of ``flat`` that ``adam_step(ema_decay=...)`` keeps, as a copy of
        ``flat`` as it is now (call it after init or load), and the device float32[2] [d_t, 1 - d_t] its launches hand over."""
        if self.ema is None:
            self.ema = self.flat.clone()
            self._ema_state = torch.zeros(2, dtype=torch.float32, device=self.device)
        return self.ema

    def adam_step(self, lr=1e-3, beta1=0.5, beta2=0.999, eps=1e-7, grad_scale=1.0, schedule=None, max_norm=None, guard=False,
                  ema_decay=None):
        """tf.keras.optimizers.Adam.apply_gradients (model.py:199-200) over the whole network: one launch.  ``schedule``: a
        device int64[3] [steps_per_epoch, epoch_step, epochs] -- ``lr`` is then the base rate of the linear decay of
        model.py:223, evaluated on the device from ``iterations`` (K.adam_sched); None: ``lr`` as it is.  ``max_norm`` (clip
        the gradient's global L2 norm to it) and ``guard`` (skip the update when the gradient holds a NaN or Inf) send the
        step through K.adam_guard instead, which decides on the device; clipping implies the skip, since a non-finite norm
        has no clip factor.  With neither, the launches are the ones above and nothing else.  ``ema_decay``: the same launches
        through K.adam_ema, which also moves ``ema`` towards the new parameters (enable_ema first); a skipped update leaves
        the average alone.  None: exactly the launches above."""
        if ema_decay is not None:
            if self.ema is None:
                raise RuntimeError("adam_step(ema_decay=...): call enable_ema() first")
            rec, ws = self.guard_buffers() if max_norm is not None or guard else (None, None)
            K.adam_ema(self.flat, self.grad, self.m, self.v, self.ema, self._adam_state, self._ema_state, ema_decay, schedule, lr, beta1,
                       beta2, eps, grad_scale, rec, ws, 0.0 if max_norm is None else max_norm)
        elif max_norm is not None or guard:
            rec, ws = self.guard_buffers()
            K.adam_guard(self.flat, self.grad, self.m, self.v, self._adam_state, rec, ws, schedule, lr, beta1, beta2, eps, grad_scale,
                         0.0 if max_norm is None else max_norm)
        elif schedule is None:
            K.adam_iter(self.flat, self.grad, self.m, self.v, self._adam_state, lr, beta1, beta2, eps, grad_scale)
        else:
            K.adam_sched(self.flat, self.grad, self.m, self.v, self._adam_state, schedule, lr, beta1, beta2, eps, grad_scale)
        self.version += 1


class Adam:
    """``tf.keras.optimizers.Adam`` as the reference holds it in ``self.g_optim`` / ``self.d_optim`` (model.py:83-84,
    199-200, 205-207), bound to one network's flat parameter store: the whole update is one fused launch."""

    def __init__(self, net, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, schedule=None, clip_norm=None,
                 skip_nonfinite=False, ema_decay=None):
        self.net, self.learning_rate, self.beta_1, self.beta_2, self.epsilon = net, learning_rate, beta_1, beta_2, epsilon
        # clip_norm: clip the global L2 norm of the network's gradient to it (None or <= 0: off); skip_nonfinite: leave the
        # network and its Adam state alone for a step whose gradient holds a NaN or Inf (ParamStore.adam_step)
        self.clip_norm = float(clip_norm) if clip_norm is not None and float(clip_norm) > 0 else None
        self.skip_nonfinite = bool(skip_nonfinite)
        # ema_decay: keep the network's ParamStore.ema in the update's launches (None: off)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        # device int64[3] [steps_per_epoch, epoch_step, epochs] or None (ParamStore.adam_step): with it, learning_rate is the
        # base rate of the linear decay
        self.schedule = schedule

    @property
    def iterations(self):
        return self.net.P.iterations

    def apply_gradients(self, grads_and_vars=None, grad_scale=1.0):
        """``optimizer.apply_gradients(zip(grads, net.trainable_variables))`` (model.py:199-200).  Called without
        arguments it consumes the network's own gradient buffer (what ``sggan.train_step`` does); given (grad, var)
        pairs, the gradients are first copied over that buffer -- ``var`` must be one of ``net.trainable_variables``."""
        P = self.net.P
        if grads_and_vars is not None:
            names = P.names()
            by_ptr = {v.data_ptr(): n for n, v in zip(names, self.net.trainable_variables)}
            P.zero_grad()
            for g, v in grads_and_vars:
                name = by_ptr.get(v.data_ptr())
                if name is None:
                    raise ValueError("apply_gradients: variable does not belong to this optimizer's network")
                if g is not None:
                    P.g(name).copy_(torch.as_tensor(g, device=P.device).reshape(P.g(name).shape))
        P.adam_step(self.learning_rate, self.beta_1, self.beta_2, self.epsilon, grad_scale, self.schedule, self.clip_norm,
                    self.skip_nonfinite, self.ema_decay)


def _layer_specs(name, shape, out_ch, norm=True):
    """One conv layer's (name, shape) entries: kernel, bias, then the instance norm's gamma, beta."""
    L = [(name + "_w", shape), (name + "_b", (out_ch,))]
    return L + [(name + "_g", (out_ch,)), (name + "_beta", (out_ch,))] if norm else L


UPSAMPLES = ("deconv", "nearest", "bilinear")


def check_upsample(upsample):
    """How generator_resnet's d1 / d2 double the resolution: 'deconv' (the reference's stride-2 transposed convs) or a fixed
    'nearest' / 'bilinear' 2x resampling in front of a stride-1 conv."""
    if upsample not in UPSAMPLES:
        raise ValueError(f"upsample must be one of {', '.join(UPSAMPLES)}, got {upsample!r}")
    return upsample


def generator_param_specs(gf_dim=64, in_c=3, out_c=3, n_blocks=9, upsample="deconv"):
    """(name, shape) in Keras ``trainable_variables`` creation order of generator_resnet (module.py:219-269).  upsample other
    than "deconv": d1 / d2 are Conv2D kernels (kh,kw,in,out) -- the element counts, and with them every offset, are unchanged."""
    resize = check_upsample(upsample) != "deconv"
    L = []
    L += _layer_specs("c1", (7, 7, in_c, gf_dim), gf_dim)
    L += _layer_specs("c2", (3, 3, gf_dim, gf_dim * 2), gf_dim * 2)
    L += _layer_specs("c3", (3, 3, gf_dim * 2, gf_dim * 4), gf_dim * 4)
    for i in range(1, n_blocks + 1):
        L += _layer_specs(f"r{i}a", (3, 3, gf_dim * 4, gf_dim * 4), gf_dim * 4)
        L += _layer_specs(f"r{i}b", (3, 3, gf_dim * 4, gf_dim * 4), gf_dim * 4)
    if resize:
        L += _layer_specs("d1", (3, 3, gf_dim * 4, gf_dim * 2), gf_dim * 2)     # Conv2D kernel behind the 2x resampling: (kh,kw,in,out)
        L += _layer_specs("d2", (3, 3, gf_dim * 2, gf_dim), gf_dim)
    else:
        L += _layer_specs("d1", (3, 3, gf_dim * 2, gf_dim * 4), gf_dim * 2)     # Conv2DTranspose kernel: (kh,kw,out,in)
        L += _layer_specs("d2", (3, 3, gf_dim, gf_dim * 2), gf_dim)
    L += _layer_specs("out", (7, 7, gf_dim, out_c), out_c, norm=False)
    return L


def unet_param_specs(gf_dim=64, in_c=3, out_c=3):
    """(name, shape) in Keras ``trainable_variables`` creation order of generator_unet (module.py:125-206): per layer, in code
    order, kernel, bias, then the instance norm's gamma, beta.  e1..e8 are Conv2D (HWIO), d1..d8 Conv2DTranspose ((kh,kw,out,in))."""
    L = []
    enc = [gf_dim, gf_dim * 2, gf_dim * 4] + [gf_dim * 8] * 5
    cin = in_c
    for i, c in enumerate(enc, 1):                                  # :139-170
        L += _layer_specs(f"e{i}", (3, 3, cin, c), c)
        cin = c
    for i, c in enumerate([gf_dim * 8] * 4 + [gf_dim * 4, gf_dim * 2, gf_dim], 1):   # :172-202
        L += _layer_specs(f"d{i}", (3, 3, c, cin), c)
        cin = c
    L += _layer_specs("d8", (3, 3, out_c, cin), out_c, norm=False)  # :204-205
    return L


D_NORMS = ("instance", "spectral")


def check_d_norm(norm):
    """The discriminators' normalisation: 'instance' (the reference's) or 'spectral' (DESIGN.md 24)."""
    if norm not in D_NORMS:
        raise ValueError(f"d_norm must be one of {', '.join(D_NORMS)}, got {norm!r}")
    return norm


def discriminator_param_specs(df_dim=64, in_c=3, segment_class=34, norm="instance"):
    """Creation order of discriminator (module.py:272-318).  norm="spectral": no layer has an instance norm, so every layer is
    kernel and bias only."""
    inorm = check_d_norm(norm) == "instance"
    L = []
    L += _layer_specs("h0", (3, 3, in_c, df_dim), df_dim, norm=False)
    L += _layer_specs("h1", (3, 3, df_dim, df_dim * 2), df_dim * 2, norm=inorm)
    L += _layer_specs("h2", (3, 3, df_dim * 2, df_dim * 4), df_dim * 4, norm=inorm)
    L += _layer_specs("h3", (3, 3, df_dim * 4, df_dim * 8), df_dim * 8, norm=inorm)
    L += _layer_specs("h31", (3, 3, df_dim * 8, df_dim * 8), df_dim * 8, norm=inorm)
    L += _layer_specs("h32", (3, 3, df_dim * 8, df_dim * 8), df_dim * 8, norm=inorm)
    L += _layer_specs("h33", (3, 3, df_dim * 8, df_dim * 8), df_dim * 8, norm=inorm)
    L += _layer_specs("h4", (3, 3, df_dim * 8, segment_class), segment_class, norm=False)
    return L


def plan_buckets(P, unit_names, n_buckets):
    """Contiguous ranges of a network's flat gradient buffer, cut at layer boundaries into ``n_buckets`` groups of about equal
    size (plus, when there is more than one, the small leading layers as a bucket of their own -- below):
    [(first_unit_name, lo, hi)] in flat (= forward) order, covering [0, P.numel) exactly.  Backward visits the layers in
    reverse, so a group's gradients are complete once the backward of its FIRST unit (weight gradient included) has been queued
    -- the point at which the data-parallel step launches that bucket's all-reduce."""
    starts = [P.index[n + "_w"][0] for n in unit_names]
    assert starts == sorted(starts) and starts[0] == 0, "units must be given in flat-buffer order"
    total = P.numel
    n_buckets = max(1, min(int(n_buckets), len(unit_names)))
    cuts = [0]
    for k in range(1, n_buckets):
        target = total * k / n_buckets
        i = min(range(len(unit_names)), key=lambda j: abs(starts[j] - target))
        if i > cuts[-1]:
            cuts.append(i)
    # the group that completes LAST (the first in flat order) has nothing of the backward pass left to hide behind: cut its
    # small leading layers (the generator's stem, <= 5 % of the buffer) off as a bucket of their own, so that the exposed
    # exchange is a latency-sized one and the bulk of the group travels under those layers' backward
    if len(cuts) > 1 or n_buckets > 1:
        first_end = cuts[1] if len(cuts) > 1 else len(unit_names)
        small = [j for j in range(1, first_end) if starts[j] <= 0.05 * total]
        if small:
            cuts.insert(1, small[-1])
    ends = cuts[1:] + [len(unit_names)]
    return [(unit_names[a], starts[a], total if b == len(unit_names) else starts[b]) for a, b in zip(cuts, ends)]


# ----------------------------------------------------------------------------- layer engine
# Defaults of two per-network switches (``sggan(fuse_in_stats=..., fuse_in_bwd=...)`` / ``net.fuse_in_stats`` / ``net.fuse_in_bwd``;
# nothing here reads the environment).  fuse_in_stats: the conv epilogue emits the following instance norm's per-chunk sums.
# fuse_in_bwd: its backward counterpart (data-gradient epilogue -> norm-backward sums) -- OFF: the epilogue has to read the norm
# input tile (and the skip gradient) at the end of a grid that has nothing to overlap the burst with.  Measured at the bench shape
# (tools/bench_conv.py --ops dgrad_add,dgrad_stats,in_bwd,in_bwd_partial): 8 images +6.6 us per data gradient against 12.9 us saved
# in the norm; 16 images (the paired cycle step's launch size) +23.4 against 22.7 -- nothing left.  Kept, parity-tested, as an
# opt-in of the one-network-at-a-time sequencing; it has no paired form.
FUSE_CONV_IN_STATS = True
FUSE_CONV_IN_BWD = False
# Round 4: the same statistics epilogue exists for the transposed layers (sgg_deconv2d_fwd_stats: the stride-2 halo kernel's own STATS build)
# and for the stem (sgg_conv2d_fwd_stats on the narrow-input kernel).  Both are parity-tested and OFF: in the cycle step the transposed
# layers' epilogue costs more than the 152 us of statistics passes it removes (-0.8 % on the step: that kernel has no registers to
# spare: 32 spilled VGPRs + a second pass over the accumulators), the stem's is neutral (profiles/r04_stats_epilogues.txt).
FUSE_DECONV_IN_STATS = False
FUSE_STEM_IN_STATS = False


class _Unit:
    """One Conv2D / Conv2DTranspose call site, optionally followed by InstanceNorm (+act, +residual), or by a fused activation
    when there is no norm -- of one network (_ConvUnit) or of two networks of one shape in lockstep on a stacked batch
    (_PairUnit).  Stateless w.r.t. activations: forward returns a record that backward consumes, so one network can be applied
    several times per step.

    This class owns the sequence -- conv -> (mask) -> norm -> record, and norm backward -> (mask) -> bias, weight and data
    gradient -- with its options, record layouts and return conventions; the two kinds supply the launches: ``_conv``,
    ``_norm``, ``_norm_backward``, ``_bias_grad``, ``weight_grad``, ``_data_grad`` (and ``geom``, ``affine``, ``dropout_``).
    The layer's description (``name``, ``kind``, ``norm``, ``act``, ``leak``, ``R``, ``cout``, ...) and ``skip_grad`` are fixed
    at construction; the switches of ``net`` are read at every call (model.py sets them after the units are built).  The
    networks' layer walks see ``name``, ``skip_grad``, ``drop_layer``, ``geom``, ``forward`` and ``backward`` and never ask
    which kind they hold.

    skip_grad: the skip tensor is added BEFORE the activation, y = act(IN(conv(x)) + skip) (generator_unet d3 / d7,
    module.py:181-184,199-202).  The record then keeps y as well -- the norm backward derives act' from it -- and backward
    returns (dx, dskip), dskip being the skip path's gradient."""

    LAYER = ("name", "kind", "stride", "padding", "reflect", "norm", "act", "leak", "R", "S", "cin", "cout", "skip_grad")
    drop_layer = None           # a dropout site's layer index (generator_unet d1..d3: 0..2): the mask sits between conv and norm

    def _epilogue_stats(self, g, fuse):
        """Does this conv's epilogue deliver the (sum, sumsq) rows of its output for the norm behind it (which then skips its
        own statistics pass over the tensor)?  fuse=False -- a dropout site in training mode -- never: the epilogue would sum
        the tensor in front of the mask.  The stem's and the transposed layers' epilogues are opt-ins of their own."""
        net = self.net
        if not (fuse and self.norm and g.stats_chunks and net.fuse_in_stats):
            return False
        return net.fuse_in_stats_deconv if self.kind == "deconv" else self.R != 7 or net.fuse_in_stats_stem

    def _limits(self, gbuf, dy_partial):
        """What this kind's backward has no form for is refused here, before anything is launched."""

    def forward(self, x, residual=None, record_only=False, out=None, drop=None):
        """Returns (y, record); record = (g, x, xc, stats) [+ (y,) with skip_grad] [+ (drop,) at a dropout site], stats None for
        a layer without a norm.
        out: the caller's buffer for the layer output (layers without a norm only: the generator's last layer writes the
        fakes straight into the discriminators' stacked input).
        record_only: the caller only wants the forward record (activation checkpointing re-runs a residual block's second
        conv for its backward pass: the block's output is not needed again) -- where one launch's epilogue delivered the
        norm's sums for the whole batch, the norm's apply pass is skipped (same statistics, bit for bit) and y is None.
        drop: (stream id, sample offset) at a dropout site in training mode -- the conv output is masked in place before the
        norm reads it, and the record grows by ``drop``, which the backward needs to repeat the launch; None: no launch."""
        assert out is None or not self.norm
        assert drop is None or (self.norm and not record_only)
        assert not self.skip_grad or (self.norm and residual is not None and not record_only)
        g, xc, part, whole = self._conv(x, out, fuse=drop is None)
        if not self.norm:
            return xc, (g, x, xc, None)
        if drop is not None:
            self.dropout_(xc, drop)
        if record_only and part is not None and whole:
            return None, (g, x, xc, K.instnorm_finalize(part, xc.shape[1] * xc.shape[2], self.net.eps))
        y, stats = self._norm(xc, residual, part)
        return y, (g, x, xc, stats) + ((y,) if self.skip_grad else ()) + (() if drop is None else (drop,))

    def backward(self, rec, dy, want_dx=True, param_grads=True, gbuf=None, addend=None, dy_partial=None, next_norm=None):
        """Returns dx (None without want_dx); (dx, partial) when next_norm is given; with skip_grad (dx, dskip).
        gbuf: a gradient buffer to use instead of the network's own.  addend: added to dx (in the data gradient's store where
        the kernel has one).  dy_partial: the norm-backward partial sums of THIS unit's norm, already computed by the data
        gradient that produced dy.  next_norm = (unit, rec) of the layer that will consume the returned dx: ``partial`` is
        the first pass of its norm backward where this unit's data-gradient epilogue can make it, else None."""
        self._limits(gbuf, dy_partial)
        g, x, xc, stats, *rest = rec
        y = rest.pop(0) if self.skip_grad else None
        drop = rest[0] if rest else None
        assert not self.skip_grad or addend is None
        assert (not self.skip_grad and drop is None) or (dy_partial is None and next_norm is None)     # (neither takes a fused-statistics route)
        dskip = None
        if self.norm:
            dxc = self._norm_backward(dy, xc, stats, y, dy_partial, param_grads, gbuf)
            if self.skip_grad:
                dxc, dskip = dxc
            if drop is not None:            # dxc becomes the gradient with respect to the conv output: the forward's launch again
                self.dropout_(dxc, drop)
        else:
            if dy.dtype != xc.dtype:
                dy = dy.to(xc.dtype)
            dxc = K.act_bwd(dy, xc, self.act, self.leak) if self.act != A.ACT_NONE else dy
        if param_grads:
            # a conv bias that feeds an InstanceNorm has an identically zero gradient and is left at 0 -- unless
            # a mask sits between them: the norm no longer cancels the bias
            if drop is not None or not self.norm:
                self._bias_grad(dxc, gbuf)
            self.weight_grad(g, x, dxc, gbuf)
        dx = None
        if want_dx:
            dx = self._data_grad(g, x, dxc, addend, next_norm)
            dx = dx if next_norm is not None else dx[0]
        return (dx, dskip) if self.skip_grad else dx


class _ConvUnit(_Unit):
    """The unit of one network: every launch is the plain per-network entry."""

    def __init__(self, net, name, kind, stride=1, padding="VALID", reflect=0, norm=True, act=A.ACT_NONE, leak=0.0, skip_grad=False):
        self.net, self.name, self.kind = net, name, kind            # kind: "conv" | "deconv"
        self.stride, self.padding, self.reflect = stride, padding, reflect
        self.norm, self.act, self.leak, self.skip_grad = norm, act, leak, skip_grad
        shape = net.P.index[name + "_w"][2]
        self.R, self.S = shape[0], shape[1]
        if kind == "conv":
            self.cin, self.cout = shape[2], shape[3]
        else:                                                       # (kh,kw,out,in)
            self.cout, self.cin = shape[2], shape[3]
        self._packed = (-1, None, None)
        self._pending = None                                        # deferred weight-gradient operands (pair_wgrads)

    def flush_wgrad(self):
        """Run a deferred weight gradient whose partner never came."""
        if self._pending is not None:
            g, x, dxc = self._pending
            self._pending = None
            K.conv_wgrad(g, x, dxc, self.net.P.g(self.name + "_w"), accumulate=True)

    def geom(self, x):
        N, H, W, Cp = x.shape
        assert Cp == K.cpad(self.cin), (self.name, Cp, self.cin)
        if self.kind == "conv":
            return K.conv_geom(N, H, W, Cp, K.cpad(self.cout), self.R, self.S, self.stride, self.padding, self.reflect, x.dtype)
        return K.deconv_geom(N, H, W, Cp, K.cpad(self.cout), self.R, self.S, self.stride, x.dtype)

    def pack_dims(self):
        """(Cpad, Kpad) of the packed GEMM operands: for a deconv the equivalent conv has C = deconv out, K = deconv in
        (the stored (kh,kw,out,in) kernel is already that conv's HWIO)."""
        return (K.cpad(self.cin), K.cpad(self.cout)) if self.kind == "conv" else (K.cpad(self.cout), K.cpad(self.cin))

    def packed(self, dtype):
        P = self.net.P
        key = (P.version, dtype)
        if self._packed[0] != key:
            if self.net.conv_units():
                self.net.repack_all(dtype)               # every layer of the net in one launch
            else:
                Cp, Kp = self.pack_dims()
                wf, wd = K.pack_weights(P.p(self.name + "_w"), Cp, Kp, dtype)
                self._packed = (key, wf, wd)
        return self._packed[1], self._packed[2]

    def affine(self):
        """(gamma, beta) of this unit's norm."""
        return self.net.P.p(self.name + "_g"), self.net.P.p(self.name + "_beta")

    def dropout_(self, t, drop):
        """The dropout launch of this site, in place on t (the conv output, or the gradient with respect to the masked tensor):
        drop = (stream id, sample offset), the mask keyed by this unit's network -- its seed and its device step counter."""
        K.dropout_(t, self.net.dropout, self.net.P.iterations, self.net.seed, drop[1], drop[0])

    def _conv(self, x, out, fuse):
        """The convolution alone: (g, xc, part, whole).  part: the statistics rows of xc where _epilogue_stats says the launch
        delivers them, else None; whole: they cover the batch from one launch (here: always)."""
        g = self.geom(x)
        wf, wd = self.packed(x.dtype)
        conv, bias = self.kind == "conv", self.net.P.p(self.name + "_b")
        if self._epilogue_stats(g, fuse):
            # (a Conv2DTranspose, module.py:254-260: the stride-2 halo kernel's epilogue emits the norm's sums too)
            return (g,) + (K.conv_fwd_stats(g, x, wf, bias) if conv else K.deconv_fwd_stats(g, x, wd, bias)) + (True,)
        fused_act = A.ACT_NONE if self.norm else self.act
        xc = K.conv_fwd(g, x, wf, bias, fused_act, self.leak, out=out) if conv else K.deconv_fwd(g, x, wd, bias, fused_act, self.leak, out=out)
        return g, xc, None, False

    def _norm(self, xc, addend, part):
        return K.instnorm_forward(xc, *self.affine(), addend, self.net.eps, self.act, self.leak, skip=self.skip_grad, partial=part)

    def _norm_backward(self, dy, xc, stats, y, part, param_grads, gbuf):
        P, n = self.net.P, self.name
        if param_grads:
            dg, db = P.g(n + "_g", buf=gbuf), P.g(n + "_beta", buf=gbuf)
        else:   # gradients w.r.t. gamma/beta not wanted: send them to scratch
            dg = db = self.net.scratch_vec(K.cpad(self.cout))
        return K.instnorm_backward(dy, xc, *self.affine(), stats, dg, db, param_grads, self.act, self.leak, y=y, partial=part)

    def _bias_grad(self, dxc, gbuf):
        K.bias_grad(dxc, self.net.P.g(self.name + "_b", buf=gbuf), accumulate=True)

    def weight_grad(self, g, x, dxc, gbuf=None):
        """dW += wgrad(x, dxc).  When the net is applied twice this step (pair_wgrads) the first application's operands are
        kept and both weight gradients run as ONE launch when the second arrives (one set of split slabs, one reduce)."""
        P, n = self.net.P, self.name
        if self.kind == "conv" and g.wgrad_pair and self.net.pair_wgrads and gbuf is None:
            if self._pending is None:
                self._pending = (g, x, dxc)
            else:
                g0, x0, d0 = self._pending
                self._pending = None
                if g0.x_shape == g.x_shape:
                    K.conv_wgrad_pair(g, x0, d0, x, dxc, P.g(n + "_w"), accumulate=True)
                else:
                    K.conv_wgrad(g0, x0, d0, P.g(n + "_w"), accumulate=True)
                    K.conv_wgrad(g, x, dxc, P.g(n + "_w"), accumulate=True)
        else:
            (K.conv_wgrad if self.kind == "conv" else K.deconv_wgrad)(g, x, dxc, P.g(n + "_w", buf=gbuf), accumulate=True)

    def _data_grad(self, g, x, dxc, addend, next_norm):
        """(dx + addend, the next norm's backward sums or None)."""
        net = self.net
        wf, wd = self.packed(x.dtype)
        if self.kind == "deconv":
            dx = K.deconv_dgrad(g, dxc, wf)
            return (dx if addend is None else K.add(dx, addend.to(dx.dtype))), None
        nu, nrec = next_norm if next_norm is not None else (None, None)
        # mixed mode: the gradient handed to the NEXT norm backward stays f32 (bf16 operands in the GEMM, f32 result)
        out_f32 = bool(net.mixed and nu is not None and nu.norm and g.dgrad_mixed and dxc.dtype == torch.bfloat16)
        if addend is not None and addend.dtype != dxc.dtype and not out_f32:
            addend = addend.to(dxc.dtype)
        if (nu is not None and not out_f32 and net.fuse_in_stats and net.fuse_in_bwd and g.bwd_stats_chunks and nu.norm
                and tuple(nrec[2].shape) == g.x_shape):
            return K.conv_dgrad_stats(g, dxc, wd, addend, nrec[2], nrec[3], *nu.affine(), nu.act, nu.leak)
        return K.conv_dgrad(g, dxc, wd, addend, out_f32=out_f32), None


class _Net:
    def __init__(self, specs, dtype, device, eps, seed):
        self.dtype = dtype
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("sggan networks run on the MI355X HIP path only (device must be a cuda/hip device)")
        A.lib()                                      # fail loudly if the extension is missing
        self.eps = eps
        self.P = ParamStore(specs, self.device)
        self.seed = 0 if seed is None else int(seed)     # keys the network's own random draws (dropout masks)
        self.dropout = 0.0                               # the rate of the network's dropout sites (GeneratorUNet)
        if seed is not None:
            self.P.init_keras(seed)
        self._scratch = None
        self._tv = None
        # set by a step that applies this net exactly twice (the cycle step): weight gradients of layers that support
        # it are deferred at the first backward and run with the second as one launch (_ConvUnit.weight_grad)
        self.pair_wgrads = False
        # mixed precision (bf16 networks only): data gradients that feed an instance-norm backward are kept in f32 where the
        # kernel supports it (the residual chain) -- see sgg_conv2d_bwd_data_mixed in include/sggan.h
        self.mixed = False
        self.fuse_in_stats, self.fuse_in_bwd = FUSE_CONV_IN_STATS, FUSE_CONV_IN_BWD
        self.fuse_in_stats_deconv, self.fuse_in_stats_stem = FUSE_DECONV_IN_STATS, FUSE_STEM_IN_STATS
        self.group2 = True           # lockstep pairs: both networks' generic convolutions in one grouped launch (sgg_*_group2)
        # activation checkpointing (BASELINE.json configs[4]): a generator keeps only each residual block's INPUT and re-runs
        # the block's two convs + norms in backward (_ResNetWalk.forward / _block_records)
        self.checkpoint_blocks = False
        self._pack_tables = {}

    def conv_units(self):
        return ()

    def adopt_seed(self, seed):
        """Take over another replica's seed, the key of this network's draws (sggan.enable_data_parallel)."""
        self.seed = int(seed)

    def repack_all(self, dtype):
        """Pack the GEMM operands of every conv layer from the current parameters with ONE launch (all of them go stale
        together at each optimizer step); buffers and the device-side item table are built once per dtype."""
        units = self.conv_units()
        st = self._pack_tables.get(dtype)
        if st is None:
            entries = [(self.P.p(u.name + "_w"),) + u.pack_dims() + (True, True) for u in units]
            st = K.pack_weights_batch(entries, dtype, self.device)
            self._pack_tables[dtype] = st
        table, n, max_elems, bufs = st
        K.repack_batch(table, n, max_elems, dtype, scale=self.pack_scale())
        key = (self.P.version, dtype)
        for u, (wf, wd) in zip(units, bufs):
            u._packed = (key, wf, wd)

    def pack_scale(self):
        """A device f32 factor per conv layer (conv_units order) that the pack multiplies into the kernels, or None."""
        return None

    def spectral_step(self):
        """A spectrally normalised network advances its power iteration here (Discriminator); every other network: nothing."""

    def spectral_grad(self, gbuf=None):
        """... and turns the gradient with respect to W / sigma into the gradient with respect to W here."""

    def spectral_state(self):
        return None

    def flush_wgrads(self):
        for u in self.conv_units():
            u.flush_wgrad()

    def pending_wgrads(self):
        return [u.name for u in self.conv_units() if u._pending is not None]

    def bucket_plan(self, n_buckets):
        """plan_buckets() over this network's layers."""
        return plan_buckets(self.P, [u.name for u in self.conv_units()], n_buckets)

    def scratch_vec(self, n):
        if self._scratch is None or self._scratch.numel() < n:
            self._scratch = torch.zeros(max(n, 1024), dtype=torch.float32, device=self.device)
        return self._scratch[:n]

    # reference-style accessors (model.py:196-200 use .trainable_variables)
    @property
    def trainable_variables(self):
        """Real-shaped views into the flat parameter buffer, in Keras creation order."""
        if self._tv is None:
            self._tv = [self.P.p(n, padded=False) for n in self.P.names()]
        return self._tv

    def requires_grad_(self, flag=True):
        """Opt the parameter views into torch autograd (only needed by tape-style callers of __call__)."""
        for v in self.trainable_variables:
            v.requires_grad_(flag)
        return self

    def to_internal(self, x, out=None):
        """(N,H,W,C_real) float32 -> channel-padded activation tensor in the network dtype (no-op if already internal).
        out: write (or copy) into the caller's buffer -- a slice of a stacked batch."""
        if x.dtype == self.dtype and x.shape[-1] % A.CPAD == 0:
            return x if out is None else out.copy_(x)
        return K.pad_channels(x.to(device=self.device, dtype=torch.float32).contiguous(), K.cpad(x.shape[-1]), self.dtype, out=out)


class _BlockInput:
    """Tape entry of a residual block under activation checkpointing: only the block's input tensor."""
    __slots__ = ("x",)

    def __init__(self, x):
        self.x = x


# One walk per topology, written against the unit protocol (_Unit): a network class hands it _ConvUnits, its lockstep pair class
# (GeneratorPair, GeneratorUNetPair, DiscriminatorPair) the _PairUnits over two networks' units -- nothing else differs, and the
# units share one forward and one backward, so a network and its pair visit the layers, report them to on_unit_done and order
# each layer's launches alike by construction.
class _ResNetWalk:
    """generator_resnet (module.py:219-269) over ``head`` (three stem units), ``blocks`` ((a, b) unit pairs of the residual
    blocks) and ``tail`` (two transposed units + the output unit); ``checkpoint_blocks`` selects activation checkpointing.
    ``upsample`` other than "deconv" (DESIGN.md 29): the two doubling units are stride-1 SAME convs and the walk puts the fixed 2x
    resampling K.upsample2x in front of each -- one launch on whatever batch the walk carries, so a lockstep pair's stacked batch
    takes one for both networks -- and its adjoint K.upsample2x_bwd behind each one's data gradient.  The unit's record holds the
    resampled tensor (its conv's input: the weight gradient reads it), which nothing else keeps alive."""

    upsample = "deconv"

    def conv_units(self):
        return self.head + [u for pair in self.blocks for u in pair] + self.tail

    def forward(self, x, out=None):
        """x: internal (N,H,W,8).  Returns (fake internal (N,H,W,8), tape).  out: buffer for the result (the step hands in
        its slice of the discriminators' stacked input).  tape: one record per stem unit, one entry per block ((ra, rb), or
        the block's input under checkpointing), one record per tail unit."""
        tape = []
        h = x
        for u in self.head:
            h, r = u.forward(h)
            tape.append(r)
        for ua, ub in self.blocks:
            y, ra = ua.forward(h)
            hin = h
            h, rb = ub.forward(y, residual=h)                 # IN(conv(y)) + x   (:216-217)
            tape.append(_BlockInput(hin) if self.checkpoint_blocks else (ra, rb))
        for u in self.tail:
            if self.upsample != "deconv" and u is not self.tail[-1]:
                h = K.upsample2x(h, self.upsample)
            h, r = u.forward(h, out=out if u is self.tail[-1] else None)
            tape.append(r)
        return h, tape

    def _block_records(self, ua, ub, rec):
        """(ra, rb) of the residual block (ua, ub): as saved by forward, or -- activation checkpointing -- recomputed from the
        block's saved input (the kernels are bitwise reproducible, so the records, and with them every gradient, are the same bits)."""
        if not isinstance(rec, _BlockInput):
            return rec
        y, ra = ua.forward(rec.x)
        _, rb = ub.forward(y, residual=rec.x, record_only=True)
        return ra, rb

    def backward(self, tape, dy, want_dx=False, param_grads=True, gbuf=None, on_unit_done=None, addend=None):
        """on_unit_done(name): called after each layer's backward (its weight gradient included) has been queued -- the
        data-parallel step hangs its per-bucket all-reduce launches on it (``bucket_plan``).  addend: a tensor shaped like the
        input gradient, added to it in the first layer's data-gradient store (the step's gradient joins: no extra pass)."""
        done = on_unit_done if on_unit_done is not None else (lambda name: None)
        nh, nt = len(self.head), len(self.tail)
        d = dy
        for u, r in zip(reversed(self.tail), reversed(tape[len(tape) - nt:])):
            d = u.backward(r, d, True, param_grads, gbuf)
            if self.upsample != "deconv" and u is not self.tail[-1]:
                d = K.upsample2x_bwd(d, self.upsample)
            done(u.name)
        # residual blocks: each data gradient also makes the first pass of the norm backward that consumes it (the
        # norm of the conv before it in forward order), so that norm skips its statistics pass over the tensor
        part = None
        blocks = [(ua, ub, rec) for (ua, ub), rec in zip(self.blocks, tape[nh:len(tape) - nt])][::-1]
        ahead = self._block_records(*blocks[0]) if blocks else None
        for k, (ua, ub, _) in enumerate(blocks):
            ra, rb = ahead
            # (the records of the block in front: its second norm consumes this block's data gradient -- under checkpointing
            # they are recomputed one block ahead, so at most two blocks' activations are alive)
            if k + 1 < len(blocks):
                ahead = self._block_records(*blocks[k + 1])
                nxt = (blocks[k + 1][1], ahead[1])
            else:
                ahead, nxt = None, (self.head[-1], tape[nh - 1])
            t, pa = ub.backward(rb, d, True, param_grads, gbuf, dy_partial=part, next_norm=(ua, ra))
            done(ub.name)
            d, part = ua.backward(ra, t, True, param_grads, gbuf, addend=d, dy_partial=pa, next_norm=nxt)   # + skip gradient (fused)
            done(ua.name)
        ra = rb = None
        for u, r in zip(reversed(self.head), reversed(tape[:nh])):
            first = u is self.head[0]
            d = u.backward(r, d, want_dx or not first, param_grads, gbuf, addend=addend if first else None, dy_partial=part)
            part = None
            done(u.name)
        return d


class Generator(_ResNetWalk, _Net):
    """generator_resnet (module.py:219-269): c7s1-64, d128, d256, 9 x R256, u128, u64, c7s1-3 + tanh."""

    def __init__(self, gf_dim=64, in_c=3, out_c=3, n_blocks=9, dtype=torch.bfloat16, device="cuda", eps=1e-3, seed=19,
                 upsample="deconv"):
        """upsample="nearest" | "bilinear" (DESIGN.md 29): u128 and u64 become the 2x resampling + a 3x3 stride-1 SAME conv +
        IN + ReLU instead of the stride-2 transposed conv + IN + ReLU."""
        super().__init__(generator_param_specs(gf_dim, in_c, out_c, n_blocks, upsample), dtype, device, eps, seed)
        self.in_c, self.out_c, self.n_blocks, self.upsample = in_c, out_c, n_blocks, upsample
        U = lambda *a, **k: _ConvUnit(self, *a, **k)
        self.c1 = U("c1", "conv", reflect=3, act=A.ACT_RELU)                       # :230-234
        self.c2 = U("c2", "conv", stride=2, padding="SAME", act=A.ACT_RELU)        # :236-238
        self.c3 = U("c3", "conv", stride=2, padding="SAME", act=A.ACT_RELU)        # :240-242
        self.blocks = [(U(f"r{i}a", "conv", reflect=1, act=A.ACT_RELU),            # residule_block :208-217
                        U(f"r{i}b", "conv", reflect=1, act=A.ACT_NONE)) for i in range(1, n_blocks + 1)]
        if upsample == "deconv":
            self.d1 = U("d1", "deconv", stride=2, act=A.ACT_RELU)                  # :254-256
            self.d2 = U("d2", "deconv", stride=2, act=A.ACT_RELU)                  # :258-260
        else:                                                                      # (the walk resamples in front of each)
            self.d1 = U("d1", "conv", padding="SAME", act=A.ACT_RELU)
            self.d2 = U("d2", "conv", padding="SAME", act=A.ACT_RELU)
        self.out = U("out", "conv", reflect=3, norm=False, act=A.ACT_TANH)         # :262-265
        self.head, self.tail = [self.c1, self.c2, self.c3], [self.d1, self.d2, self.out]

    def __call__(self, x, training=False):
        """Drop-in for ``self.generator(self.real_A)`` (model.py:175): NHWC float32 in, NHWC float32 out.  training: Keras's
        keyword -- the U-Net's dropout layers mask (application 0, sample offset 0); a network without dropout layers ignores it."""
        return _apply_net(self, x, *((True,) if training else ()))

    def _run(self, x, training=False):
        y, tape = self.forward(self.to_internal(x))
        return K.unpad_channels(y, self.out_c), tape

    def _run_backward(self, tape, dy_real, gbuf, want_dx):
        dy = K.pad_channels(dy_real.contiguous(), K.cpad(self.out_c), self.dtype)
        dx = self.backward(tape, dy, want_dx, True, gbuf)
        return None if dx is None else K.unpad_channels(dx, self.in_c)


class _UNetWalk:
    """generator_unet (module.py:125-206) over ``enc`` (the encoder units), ``dec`` (the decoder units that take a skip: one
    fewer, the last encoder output being the decoder's input) and ``d8`` (the output unit)."""

    def conv_units(self):
        return self.enc + self.dec + [self.d8]

    def forward(self, x, out=None, dropout=None, sample_offset=0):
        """x: internal (N,H,W,8).  Returns (fake internal (N,H,W,8), tape); out: buffer for the result.  tape = the layers'
        forward records in layer order.
        dropout: None -- inference, the dropout layers are the identity -- or the index of this application of the network within
        the step (training mode): dropout site l then masks its conv output with draw stream 4 * application + l, sample i of
        the batch being global sample ``sample_offset`` + i.  Forward and backward of one application must run at the same value
        of the network's step counter."""
        tape, skips = [], []
        h = x
        for u in self.enc:
            h, r = u.forward(h)
            tape.append(r)
            skips.append(h)
        skips.pop()                                            # (the innermost output feeds the decoder: no skip)
        for u in self.dec:                                     # d(j) + e(8-j): the skips are consumed innermost first
            if dropout is not None and u.drop_layer is not None:
                h, r = u.forward(h, residual=skips.pop(), drop=(4 * int(dropout) + u.drop_layer, int(sample_offset)))
            else:
                h, r = u.forward(h, residual=skips.pop())
            tape.append(r)
        h, r = self.d8.forward(h, out=out)
        tape.append(r)
        return h, tape

    def backward(self, tape, dy, want_dx=False, param_grads=True, gbuf=None, on_unit_done=None, addend=None):
        """on_unit_done, addend: as the ResNet walk's.  The decoder produces the skip gradients (units with ``skip_grad``, d3 / d7:
        dy * relu'(y) from the norm backward; the others: the gradient of the layer's output itself); each is held until the
        encoder's backward reaches its layer and joins that layer's gradient in the data-gradient store of the conv behind it."""
        done = on_unit_done if on_unit_done is not None else (lambda name: None)
        ne = len(self.enc)
        d = self.d8.backward(tape[-1], dy, True, param_grads, gbuf)
        done(self.d8.name)
        joins = [addend]            # what each encoder unit's data-gradient store adds, outermost first: the step's join, then the skips
        for u, r in zip(reversed(self.dec), reversed(tape[ne:-1])):
            if u.skip_grad:
                d, dskip = u.backward(r, d, True, param_grads, gbuf)
            else:
                dskip = d
                d = u.backward(r, d, True, param_grads, gbuf)
            joins.append(dskip)
            done(u.name)
        dskip = None
        for u, r in zip(reversed(self.enc), reversed(tape[:ne])):
            d = u.backward(r, d, want_dx or u is not self.enc[0], param_grads, gbuf, addend=joins.pop())   # + skip gradient (fused store)
            done(u.name)
        return d


class GeneratorUNet(_UNetWalk, _Net):
    """generator_unet (module.py:125-206), the reference's default generator (--use_resnet False): eight 3x3 stride-1 SAME
    Conv2D + IN + LeakyReLU (e8: ReLU), seven 3x3 stride-1 SAME Conv2DTranspose + IN + additive skip from the mirrored
    encoder layer (d3 / d7: ReLU after the add), and a Conv2DTranspose to the output channels + tanh.

    Dropout(``dropout``) sits between the Conv2DTranspose and the instance norm of d1, d2 and d3 (module.py:170, 175, 180; the
    reference's constant, :131, is the default).  In inference mode -- ``generator(x)``, ``forward(x)``: what the reference's own
    calls run, since it calls the generator without ``training=`` (model.py:173-178, 347, 561) -- the three layers are the
    identity and nothing is launched for them.  In training mode -- ``generator(x, training=True)``, ``forward(x, dropout=
    application)`` -- each masks its conv output in place (K.dropout_): the mask is regenerated from (seed, the
    network's device step counter, application, layer, global sample index, element index) in forward and backward, never
    stored, and the biases d1_b, d2_b, d3_b get the gradient the norm would otherwise cancel."""

    LEAK = 0.3           # tf.keras.layers.LeakyReLU() default alpha

    def __init__(self, gf_dim=64, in_c=3, out_c=3, dtype=torch.bfloat16, device="cuda", eps=1e-3, seed=19, dropout=0.5):
        super().__init__(unet_param_specs(gf_dim, in_c, out_c), dtype, device, eps, seed)
        self.in_c, self.out_c = in_c, out_c
        K.dropout_threshold(dropout)                    # (0 <= rate < 1, else ValueError)
        self.dropout = float(dropout)
        U = lambda *a, **k: _ConvUnit(self, *a, padding="SAME", **k)
        self.enc = [U(f"e{i}", "conv", act=A.ACT_LRELU, leak=self.LEAK) for i in range(1, 8)] + [U("e8", "conv", act=A.ACT_RELU)]
        self.dec = [(U(f"d{i}", "deconv", stride=1, act=A.ACT_RELU, skip_grad=True) if i in (3, 7) else     # (ReLU after the add)
                     U(f"d{i}", "deconv", stride=1, act=A.ACT_NONE)) for i in range(1, 8)]
        self.d8 = U("d8", "deconv", stride=1, norm=False, act=A.ACT_TANH)
        for layer, u in enumerate(self.dec[:3]):        # d1, d2, d3: the dropout sites (:170, :175, :180)
            u.drop_layer = layer

    def _run(self, x, training=False):
        y, tape = self.forward(self.to_internal(x), dropout=0 if training else None)
        return K.unpad_channels(y, self.out_c), tape

    __call__ = Generator.__call__
    _run_backward = Generator._run_backward


class _DiscriminatorWalk:
    """discriminator (module.py:272-318) over ``units`` (the convs with an activation) and ``h4`` (the class-logit conv), then
    the mask multiply and channel sum (``segment_class`` channels, activations in ``dtype``)."""

    def conv_units(self):
        return list(self.units) + [self.h4]

    def forward(self, x, mask):
        """x internal (N,H,W,8); mask f32 (N,mh,mw,segment_class).  Returns (logits f32 (N,mh,mw,1), tape): one record per
        unit, then (mask, h4's shape)."""
        tape = []
        h = x
        for u in self.conv_units():
            h, r = u.forward(h)
            tape.append(r)
        mask = mask.to(device=h.device, dtype=torch.float32).contiguous()
        out = K.mask_reduce_fwd(h, mask, self.segment_class)                     # :312-314
        tape.append((mask, tuple(h.shape)))
        return out, tape

    def backward(self, tape, dlogits, want_dx=False, param_grads=True, gbuf=None, addend=None, feature_addends=None):
        """addend: added to the image gradient in the first unit's data-gradient store (as in the generators' walks).
        feature_addends: one tensor per entry of ``features(tape)``; entry k, the gradient of a loss on feature k,
        joins the walk's gradient of that feature where it is made -- in the data-gradient store of unit k + 1, its consumer,
        exactly as ``addend`` joins the image gradient in h0's.  None: the walk as it always was, call for call."""
        *recs, (mask, h4_shape) = tape
        d = K.mask_reduce_bwd(dlogits.contiguous(), mask, h4_shape, self.dtype, self.segment_class)
        units = self.conv_units()
        joins = [addend] + (list(feature_addends) if feature_addends is not None else [None] * (len(units) - 1))
        assert len(joins) == len(units), f"feature_addends: {len(units) - 1} tensors, one per feature"
        for u, r in zip(reversed(units), reversed(recs)):
            first = u is units[0]
            d = u.backward(r, d, want_dx or not first, param_grads, gbuf, addend=joins.pop())
        return d

    def features(self, tape, lo=None, hi=None):
        """The intermediate activations of a pass: the outputs of h0 .. h33 -- post-activation, each already
        materialised as the recorded input of the unit behind it (h1 .. h33, h4) -- of images [lo, hi), as views, sliced like
        ``slice_tape``.  h4's output, the logit map, is not a feature."""
        *recs, _ = tape
        return [r[1][lo:hi] for r in recs[1:]]

    def slice_tape(self, tape, lo, hi):
        """The forward records of images [lo, hi) of a pass, as views (a backward pass through part of the batch: the step sends
        reals and fakes through D as one stacked pass, the generator's loss only needs the fakes).  Of a lockstep pair's stacked
        pass the slice must hold as many images of the first network as of the second."""
        *recs, (mask, h4_shape) = tape
        out = []
        for u, (g, x, xc, stats) in zip(self.conv_units(), recs):
            xs = x[lo:hi]
            out.append((u.geom(xs), xs, xc[lo:hi], None if stats is None else stats[lo:hi]))
        out.append((mask[lo:hi], (hi - lo,) + tuple(h4_shape[1:])))
        return out


class Discriminator(_DiscriminatorWalk, _Net):
    """discriminator (module.py:272-318): 8 convs, mask multiply, channel sum."""

    def __init__(self, df_dim=64, in_c=3, segment_class=34, dtype=torch.bfloat16, device="cuda", eps=1e-3, leak=0.3, seed=20,
                 norm="instance"):
        """norm="spectral" (DESIGN.md 24): h1..h33 lose their instance norm -- they become conv + LeakyReLU units like h0, their
        bias now has a gradient -- and every layer runs on W / sigma(W), sigma being the estimate of W's largest singular value
        that one power iteration per training step (spectral_step) keeps in a persistent vector u per layer."""
        super().__init__(discriminator_param_specs(df_dim, in_c, segment_class, norm), dtype, device, eps, seed)
        self.in_c, self.segment_class, self.norm = in_c, segment_class, norm
        inorm = norm == "instance"
        U = lambda *a, **k: _ConvUnit(self, *a, act=A.ACT_LRELU, leak=leak, **k)
        self.units = [U("h0", "conv", stride=2, padding="SAME", norm=False),      # :284-285
                      U("h1", "conv", stride=2, padding="SAME", norm=inorm),      # :287-289
                      U("h2", "conv", stride=2, padding="SAME", norm=inorm),      # :291-293
                      U("h3", "conv", stride=1, padding="SAME", norm=inorm),      # :295-297
                      U("h31", "conv", stride=2, padding="VALID", norm=inorm),    # :299-301
                      U("h32", "conv", stride=2, padding="VALID", norm=inorm),    # :303-305
                      U("h33", "conv", stride=1, padding="VALID", norm=inorm)]    # :307-309
        self.h4 = _ConvUnit(self, "h4", "conv", stride=1, padding="SAME", norm=False, act=A.ACT_NONE)   # :311
        self._sn = None
        if not inorm:
            self._init_spectral(seed)

    # ------------------------------------------------------------------ spectral norm
    def _init_spectral(self, seed):
        """Per layer (conv_units order): u (K), v (R*S*C), sigma and 1 / sigma, all f32 on the device, in four flat buffers (every
        vector starts on a 16-byte boundary), and the item table over them, the kernels and this network's own gradient buffer.
        u: a normal draw from the network's seed, l2-normalised."""
        P, dev = self.P, self.device
        mats = [tuple(int(d) for d in (np.prod(P.index[u.name + "_w"][2][:-1]), P.index[u.name + "_w"][2][-1])) for u in self.conv_units()]
        pad4 = lambda n: (n + 3) // 4 * 4
        uo, vo = np.cumsum([0] + [pad4(k) for _, k in mats]), np.cumsum([0] + [pad4(r) for r, _ in mats])
        sn = self._sn = SimpleNamespace(mats=mats, uo=uo, vo=vo)
        sn.u0 = host = self._seeded_u(seed)                                      # (the seeded start: a checkpoint without u resumes from it)
        sn.u = host.to(dev)
        sn.v = torch.zeros(int(vo[-1]), dtype=torch.float32, device=dev)
        sn.sigma = torch.ones(len(mats), dtype=torch.float32, device=dev)
        sn.inv_sigma = torch.ones(len(mats), dtype=torch.float32, device=dev)
        sn.table = K.SpectralTable(self._spectral_entries(P.grad), dev)
        sn.seen = None               # P.loaded at the time sigma was last computed (None: never)

    def _seeded_u(self, seed):
        """The seeded start of the u vectors, flat on the host: a function of the seed and the layers' widths alone."""
        sn = self._sn
        gen = torch.Generator(device="cpu").manual_seed(int(seed if seed is not None else 0) + 7919)
        host = torch.zeros(int(sn.uo[-1]), dtype=torch.float32)
        for (_, k), o in zip(sn.mats, sn.uo):
            d = torch.randn(k, generator=gen, dtype=torch.float64)
            host[o:o + k] = (d / d.norm()).to(torch.float32)
        return host

    def adopt_seed(self, seed):
        """... and, with it, the seeded start of u.  The vectors in use are not touched."""
        super().adopt_seed(seed)
        if self._sn is not None:
            self._sn.u0 = self._seeded_u(seed)

    def _spectral_entries(self, gbuf):
        sn, P = self._sn, self.P
        out = []
        for i, (unit, (rows, k)) in enumerate(zip(self.conv_units(), sn.mats)):
            n = unit.name + "_w"
            out.append((P.p(n).view(rows, k), P.g(n, buf=gbuf).view(rows, k), sn.u[sn.uo[i]:sn.uo[i] + k], sn.v[sn.vo[i]:sn.vo[i] + rows],
                        sn.sigma[i:i + 1], sn.inv_sigma[i:i + 1]))
        return out

    def spectral_step(self):
        """One power iteration per layer on the current parameters: u, v, sigma and 1 / sigma move, and the packed operands go
        stale, so that every forward and gradient up to the next call runs on W / sigma with this sigma.  The step bodies call
        it once per training step, before the network's first use."""
        if self._sn is not None:
            K.spectral_sigma(self._sn.table, advance=True)
            self._sn.seen = self.P.loaded
            self.P.version += 1

    def pack_scale(self):
        """1 / sigma per layer for the pack.  A network whose parameters were just initialised or loaded has no sigma yet: it
        is computed from u as it stands, without advancing u."""
        sn = self._sn
        if sn is None:
            return None
        if sn.seen != self.P.loaded:
            K.spectral_sigma(sn.table, advance=False)
            sn.seen = self.P.loaded
        return sn.inv_sigma

    def spectral_grad(self, gbuf=None):
        """The kernels' gradients are with respect to W / sigma: dW = (dWbar - <dWbar, W / sigma> v ut) / sigma, in place on the
        kernel slices of the gradient buffer (this network's own, or ``gbuf``).  Linear in dWbar, so once per accumulated buffer."""
        if self._sn is not None:
            K.spectral_grad(self._sn.table if gbuf is None else K.SpectralTable(self._spectral_entries(gbuf), self.device))

    def spectral_state(self):
        """The u vectors, per layer in one flat device buffer (None for an instance-norm network)."""
        return None if self._sn is None else self._sn.u

    def set_spectral_state(self, u=None):
        """Replace the u vectors (a flat buffer as spectral_state gives it; None: the seeded start); sigma is computed anew."""
        sn = self._sn
        sn.u.copy_(sn.u0 if u is None else u)
        sn.seen = None
        self.P.version += 1

    def spectral_vectors(self):
        """{layer: (u, v, sigma, 1 / sigma)} as host float32 arrays / floats (tests, logging; synchronises)."""
        sn = self._sn
        u, v, s, r = (t.cpu().numpy() for t in (sn.u, sn.v, sn.sigma, sn.inv_sigma))
        return {unit.name: (u[sn.uo[i]:sn.uo[i] + k].copy(), v[sn.vo[i]:sn.vo[i] + rows].copy(), float(s[i]), float(r[i]))
                for i, (unit, (rows, k)) in enumerate(zip(self.conv_units(), sn.mats))}

    def out_hw(self, H, W):
        """Spatial size of the h4 map for an HxW input (deviation D1: the mask grid to use above 128x128)."""
        def sz(n):
            for _ in range(3):
                n = -(-n // 2)
            n = (n - 3) // 2 + 1
            n = (n - 3) // 2 + 1
            return n - 2
        return sz(H), sz(W)

    def __call__(self, inputs):
        """Drop-in for ``self.discriminator([image, mask])`` (model.py:186-188)."""
        x, mask = inputs
        return _apply_net(self, x, mask)

    def _run(self, x, mask):
        return self.forward(self.to_internal(x), mask)

    def _run_backward(self, tape, dlogits, gbuf, want_dx):
        dx = self.backward(tape, dlogits, want_dx, True, gbuf)
        return None if dx is None else K.unpad_channels(dx, self.in_c)


# ----------------------------------------------------------------------------- two networks in lockstep
class _PairUnit(_Unit):
    """The same call site of TWO networks of one shape (G_A->B / G_B->A, D_A / D_B), applied to a batch that stacks their
    activations: images [:n] belong to ``ua``'s network, [n:] to ``ub``'s.  The convolutions run with each network's weights --
    one stacked or grouped launch where the kernel has such a form, else per half into slices of one stacked output; the
    instance norm -- per image -- runs ONCE over the stacked tensor with the affine parameters picked by image index
    (sgg_instnorm_*_pair): twice the bytes per launch (a 67 MB pass reaches 5-5.5 TB/s, a 33 MB one 4.1-4.5), half the
    launches, and per image exactly the arithmetic of two separate calls.  The first network's switches govern the pair."""

    def __init__(self, ua, ub):
        assert [getattr(ua, f) for f in self.LAYER] == [getattr(ub, f) for f in self.LAYER]
        self.ua, self.ub = ua, ub
        for f in self.LAYER:
            setattr(self, f, getattr(ua, f))

    net = property(lambda self: self.ua.net)
    drop_layer = property(lambda self: self.ua.drop_layer)

    def _limits(self, gbuf, dy_partial):
        """The lockstep path's limits: gradients go to the networks' own buffers, the data-gradient epilogue never makes a
        norm's backward sums (fuse_in_bwd has no paired form, so none can arrive and ``partial`` is None on the way out), and
        mixed mode runs one network at a time."""
        assert gbuf is None and dy_partial is None and not (self.ua.net.mixed or self.ub.net.mixed)

    def _halves(self, t):
        """((unit, the slice of its network's images in the stacked tensor t), ...)."""
        n = t.shape[0] // 2
        return (self.ua, slice(0, n)), (self.ub, slice(n, 2 * n))

    def geom(self, x):
        """The per-network geometry of a stacked batch: each network convolves its half."""
        return self.ua.geom(x[:x.shape[0] // 2])

    def affine(self):
        """(gamma, beta) of the first network's norm, then the second's."""
        return self.ua.affine() + self.ub.affine()

    def dropout_(self, t, drop):
        """Each network masks its own images with its own seed and step counter (two launches): exactly the launches of the
        one-network-at-a-time step."""
        for u, sl in self._halves(t):
            u.dropout_(t[sl], drop)

    def _conv(self, x, out, fuse):
        """The convolution of both halves into one stacked output: (g, xc, part, whole).  part: the statistics rows of xc
        where _epilogue_stats says the launches deliver them, else None; whole: they came from ONE launch over the stacked
        batch (the two networks' 3x3 halo kernel), not from one launch per half."""
        ua, ub = self.ua, self.ub
        n = x.shape[0] // 2
        g = self.geom(x)
        conv = self.kind == "conv"
        stats = self._epilogue_stats(g, fuse)
        gs = ua.geom(x) if stats else None                     # the stacked batch: one launch with per-image weights
        if stats and conv and not gs.pair_ok:                  # no such form: one launch per network
            xc = torch.empty((2 * n,) + tuple(g.y_shape[1:]), dtype=x.dtype, device=x.device)
            part = torch.empty((2 * n, g.stats_chunks, g.y_shape[3], 2), dtype=torch.float32, device=x.device)
            for u, sl in self._halves(x):
                K.conv_fwd_stats(g, x[sl], u.packed(x.dtype)[0], u.net.P.p(self.name + "_b"), out=xc[sl], out_partial=part[sl])
            return g, xc, part, False
        (wfa, wda), (wfb, wdb) = ua.packed(x.dtype), ub.packed(x.dtype)
        ba, bb = ua.net.P.p(self.name + "_b"), ub.net.P.p(self.name + "_b")
        if stats and conv:
            # the 3x3 halo kernel: 512 blocks, the second round's halo loads run under the first round's stores
            return (g,) + K.conv_fwd_stats_pair(gs, x, wfa, ba, wfb, bb, n) + (True,)
        if stats and self.net.group2:                          # (the transposed layers' stride-2 halo kernel)
            return (g,) + K.deconv_fwd_stats(gs, x, wda, ba, pair=(wdb, bb, n)) + (False,)
        # every other convolution: ONE grouped launch for both networks (sgg_*_group2: each network's call as its own group of
        # blocks -- bit-identical to two calls; the discriminators' small maps are latency bound, two half-size launches cost twice)
        fused_act = A.ACT_NONE if self.norm else self.act
        if not self.net.group2:                               # A/B switch: one launch per network into slices of the stacked output
            xc = K._out(out, (2 * n,) + tuple(g.y_shape[1:]), x.dtype, x.device)
            for (u, sl), w, bias in zip(self._halves(x), (wfa if conv else wda, wfb if conv else wdb), (ba, bb)):
                (K.conv_fwd if conv else K.deconv_fwd)(g, x[sl], w, bias, fused_act, self.leak, out=xc[sl])
        elif conv:
            xc = K.conv_fwd_group2(g, x, wfa, ba, wfb, bb, fused_act, self.leak, out=out)
        else:
            xc = K.deconv_fwd_group2(g, x, wda, ba, wdb, bb, fused_act, self.leak, out=out)
        return g, xc, None, False

    def _norm(self, xc, addend, part):
        ga, ba, gb, bb = self.affine()
        return K.instnorm_forward(xc, ga, ba, addend, self.net.eps, self.act, self.leak, skip=self.skip_grad, partial=part,
                                  pair=(gb, bb, xc.shape[0] // 2))

    def _norm_backward(self, dy, xc, stats, y, part, param_grads, gbuf):
        ua, ub = self.ua, self.ub
        ga, ba, gb, bb = self.affine()
        if param_grads:
            dga, dba, dgb, dbb = (u.net.P.g(self.name + k) for u in (ua, ub) for k in ("_g", "_beta"))
        else:   # gradients w.r.t. gamma / beta not wanted: send them to scratch
            dga = dba = ua.net.scratch_vec(K.cpad(self.cout))
            dgb = dbb = ub.net.scratch_vec(K.cpad(self.cout))
        return K.instnorm_backward(dy, xc, ga, ba, stats, dga, dba, param_grads, self.act, self.leak, y=y,
                                   pair=(gb, bb, xc.shape[0] // 2, dgb, dbb))

    def _bias_grad(self, dxc, gbuf):
        """As the one-network units take theirs (bit-identical per half)."""
        if self.net.group2:
            K.bias_grad_group2(dxc, self.ua.net.P.g(self.name + "_b"), self.ub.net.P.g(self.name + "_b"), accumulate=True)
        else:
            for u, sl in self._halves(dxc):
                K.bias_grad(dxc[sl], u.net.P.g(self.name + "_b"), accumulate=True)

    def weight_grad(self, g, x, dxc, gbuf=None):
        """The weight gradients of both networks."""
        ua, ub = self.ua, self.ub
        (_, a), (_, b) = self._halves(x)
        xa, xb, da, db = x[a], x[b], dxc[a], dxc[b]
        dwa, dwb = ua.net.P.g(self.name + "_w"), ub.net.P.g(self.name + "_w")
        # both networks have this layer's first application waiting (pair_wgrads): all four weight gradients in ONE launch
        pa, pb = ua._pending, ub._pending
        pairable = self.kind == "conv" and g.wgrad_pair                      # the 3x3 layers' two-application form
        quad = (pairable and ua.net.pair_wgrads and ub.net.pair_wgrads and pa is not None and pb is not None
                and pa[0].x_shape == g.x_shape and pb[0].x_shape == g.x_shape)
        defer = pairable and (ua.net.pair_wgrads or ub.net.pair_wgrads)
        if quad and K.conv_wgrad_pair2(g, (pa[1], pa[2], xa, da, dwa), (pb[1], pb[2], xb, db, dwb), accumulate=True):
            ua._pending = ub._pending = None
        elif self.net.group2 and not defer and pa is None and pb is None:
            # both networks' weight gradients as one grouped call: two main kernels, one slab reduce (bit-identical to two calls)
            K.conv_wgrad_group2(g, x, dxc, dwa, dwb, accumulate=True)
        else:
            ua.weight_grad(g, xa, da)
            ub.weight_grad(g, xb, db)

    def _data_grad(self, g, x, dxc, addend, next_norm):
        """(the stacked data gradient + addend, None)."""
        ua, ub = self.ua, self.ub
        conv = self.kind == "conv"
        (wfa, wda), (wfb, wdb) = ua.packed(x.dtype), ub.packed(x.dtype)
        if conv and ua.geom(x).pair_ok:
            return K.conv_dgrad_pair(ua.geom(x), dxc, wda, wdb, x.shape[0] // 2, addend), None
        if conv and self.net.group2:
            return K.conv_dgrad_group2(g, dxc, wda, wdb, addend), None
        if conv:
            dx = torch.empty(tuple(x.shape), dtype=dxc.dtype, device=dxc.device)
            for (u, sl), wd in zip(self._halves(x), (wda, wdb)):
                K.conv_dgrad(g, dxc[sl], wd, None if addend is None else addend[sl], out=dx[sl])
            return dx, None
        if self.net.group2:
            dx = K.deconv_dgrad_group2(g, dxc, wfa, wfb)
        else:
            dx = torch.empty(tuple(x.shape), dtype=dxc.dtype, device=dxc.device)
            for (u, sl), wf in zip(self._halves(x), (wfa, wfb)):
                K.deconv_dgrad(g, dxc[sl], wf, out=dx[sl])
        return (dx if addend is None else K.add(dx, addend.to(dx.dtype))), None


def _pair_units(xs, ys):
    """The lockstep units of two networks' unit lists."""
    return [_PairUnit(ua, ub) for ua, ub in zip(xs, ys)]


class GeneratorPair(_ResNetWalk):
    """generator_resnet (module.py:219-269) of two generators in lockstep: forward([x_a; x_b]) = [G_a(x_a); G_b(x_b)] -- the
    one ResNet walk over lockstep units, on stacked tensors."""

    def __init__(self, ga, gb):
        assert (ga.n_blocks, ga.upsample) == (gb.n_blocks, gb.upsample)
        self.a, self.b, self.upsample = ga, gb, ga.upsample
        self.head, self.tail = _pair_units(ga.head, gb.head), _pair_units(ga.tail, gb.tail)
        self.blocks = [tuple(_pair_units(xa, xb)) for xa, xb in zip(ga.blocks, gb.blocks)]

    @property
    def checkpoint_blocks(self):
        return self.a.checkpoint_blocks or self.b.checkpoint_blocks


class GeneratorUNetPair(_UNetWalk):
    """generator_unet (module.py:125-206) of two generators in lockstep: forward([x_a; x_b]) = [G_a(x_a); G_b(x_b)] -- the one
    U-Net walk over lockstep units: the skips and their gradients stay stacked (the gradients ride in the addend of the encoder
    convs' data-gradient store), every instance norm is one launch for both networks."""

    def __init__(self, ga, gb):
        self.a, self.b = ga, gb
        self.enc, self.dec = _pair_units(ga.enc, gb.enc), _pair_units(ga.dec, gb.dec)
        self.d8 = _PairUnit(ga.d8, gb.d8)


class DiscriminatorPair(_DiscriminatorWalk):
    """discriminator (module.py:272-318) of two discriminators in lockstep on stacked images and masks: the one discriminator
    walk over lockstep units."""

    def __init__(self, da, db):
        assert (da.segment_class, da.dtype) == (db.segment_class, db.dtype)
        self.a, self.b = da, db
        self.segment_class, self.dtype = da.segment_class, da.dtype
        self.units = _pair_units(da.units, db.units)
        self.h4 = _PairUnit(da.h4, db.h4)


# ----------------------------------------------------------------------------- autograd facade
class _NetFn(torch.autograd.Function):
    """Lets ``generator(x)`` / ``discriminator([x, mask])`` be used under torch autograd (tape-style
    callers like model.py:170-197).  The training loop of ``sggan`` does not go through this."""

    @staticmethod
    def forward(ctx, net, run_args, x, *params):
        """run_args: what the network's ``_run`` takes beside x -- (mask,) for a discriminator, () or (training,) for a generator."""
        y, tape = net._run(x, *run_args)
        ctx.net, ctx.tape = net, tape
        return y

    @staticmethod
    def backward(ctx, dy):
        net = ctx.net
        gbuf = torch.zeros_like(net.P.grad)
        dx = net._run_backward(ctx.tape, dy.to(torch.float32), gbuf, ctx.needs_input_grad[2])
        net.spectral_grad(gbuf)                      # (a spectrally normalised network: gradients with respect to the stored kernels)
        grads = tuple(net.P.g(n, buf=gbuf) for n in net.P.names())
        return (None, None, dx) + grads


def _apply_net(net, x, *run_args):
    x = torch.as_tensor(x)
    if x.device != net.device:
        x = x.to(net.device)
    params = net.trainable_variables
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        return _NetFn.apply(net, run_args, x, *params)
    y, _ = net._run(x, *run_args)
    return y


def generator_resnet(**kw) -> Generator:
    """module.py:219 -- returns a callable ``G(x)``; keyword dims default to the reference constants."""
    return Generator(**kw)


def generator_unet(**kw) -> GeneratorUNet:
    """module.py:125 -- the U-Net generator; keyword dims default to the reference constants (gf_dim 64, 3 -> 3 channels)."""
    return GeneratorUNet(**kw)


def discriminator(**kw) -> Discriminator:
    """module.py:272 -- returns a callable ``D([x, mask])``."""
    return Discriminator(**kw)
